"""GPU suite for the SM2 signature scheme (include/ecsimd_sm2.h).  Every expected value comes from tools/sm2_model.py (Python integers, its own SM3) or from
tests/golden/sm2_vectors.json (the standard's example and records adjudicated by libcrypto when the file was minted), never from the library: SM3 on the
padding boundaries (equal lengths, one length per lane, byte offset 1, rows with garbage behind the message), Z_A and e on every fixture record with shared
and per-lane identities, the fixture bit for bit through verify, verify_digest, sign_digest (both nonce modes) and pubkey, verdicts lane by lane in mixed
batches, the batch sizes around the block and the shared inversion's first two-element lane, the refused arguments, graph replay and the wiped workspace."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sm2_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
P, N = model.P, model.N
M64 = (1 << 64) - 1
SIZES = (0, 1, 63, 64, 65, 257)
TWO_PER_LANE = (1 << 18) + 1          # the shared inversion gives a lane two elements from 2^18 on; one more and the last lane holds a single one


def limbs(vals):
    return np.array([[(v >> (64 * i)) & M64 for i in range(4)] for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def dev(engine, vals):
    return engine.to_device(limbs(vals))


def ints(t):
    a = t.detach().cpu().numpy().view(np.uint64)
    return [sum(int(a[i][j]) << (64 * j) for j in range(4)) for i in range(a.shape[0])]


def flags(t):
    return t.cpu().tolist()


def rows(engine, msgs, width=None, offset=0, garbage=0xA5):
    """The byte strings as the rows of a 2-D uint8 device tensor `width` wide (the longest by default), `garbage` behind each, the whole `offset` bytes into
    its allocation; and their lengths as an int32 device tensor."""
    import torch
    n = len(msgs)
    width = max([len(m) for m in msgs] + [1]) if width is None else width
    a = np.full((n, width), garbage, dtype=np.uint8)
    for i, m in enumerate(msgs):
        a[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
    buf = torch.zeros(n * width + 8, dtype=torch.uint8, device=engine.tdev)
    view = buf[offset:offset + n * width].view(n, width)
    view.copy_(torch.from_numpy(a).to(engine.tdev))
    lens = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=engine.tdev)
    return view, lens


@functools.lru_cache(maxsize=None)
def fixture():
    return model.load_fixture()


@functools.lru_cache(maxsize=None)
def curve():
    from ecsimd_amd import Engine
    return Engine.sm2_curve()


I = lambda r, k: int(r[k], 16)


@functools.lru_cache(maxsize=None)
def message_records():
    """The message-level records, each with the model's Z_A and e."""
    out = []
    for r in fixture()["message"]:
        q, ident, msg = (I(r, "qx"), I(r, "qy")), bytes.fromhex(r["id"]), bytes.fromhex(r["msg"])
        out.append(dict(q=q, id=ident, msg=msg, r=I(r, "r"), s=I(r, "s"), ok=r["ok"], za=int(model.za(q, ident).hex(), 16), e=model.digest(q, ident, msg)))
    return out


@functools.lru_cache(maxsize=None)
def digest_lanes():
    """Every record kind as one list of (q, e, r, s, ok): the digest-level verdicts, the message records under the model's e, the signing records' signatures."""
    fx = fixture()
    out = [((I(r, "qx"), I(r, "qy")), I(r, "e"), I(r, "r"), I(r, "s"), r["ok"]) for r in fx["digest"]]
    out += [(m["q"], m["e"], m["r"], m["s"], m["ok"]) for m in message_records()]
    out += [((I(r, "qx"), I(r, "qy")), I(r, "e"), I(r, "r"), I(r, "s"), r["ok"]) for r in fx["sign"]]        # a refused signing lane is r = s = 0: invalid
    ex = fx["example"]
    out.append(((I(ex, "qx"), I(ex, "qy")), I(ex, "e"), I(ex, "r"), I(ex, "s"), 1))
    return out


@functools.lru_cache(maxsize=None)
def sign_pool(deterministic):
    """(e, d, k, r, s, ok) of the signing records: the caller-nonce ones as stored, or EVERY record's (e, d) under the deterministic nonce, from the model."""
    out = []
    for r in fixture()["sign"]:
        e, d = I(r, "e"), I(r, "d")
        if deterministic:
            out.append((e, d, None) + model.sign_digest(e, d, None))
        elif r["k"] is not None:
            out.append((e, d, I(r, "k"), I(r, "r"), I(r, "s"), r["ok"]))
    return out


@functools.lru_cache(maxsize=None)
def key_pool():
    return [(I(r, "d"), I(r, "qx"), I(r, "qy"), r["key_ok"]) for r in fixture()["sign"]]


def tile(pool, n):
    return [pool[i % len(pool)] for i in range(n)]


# ---- SM3
def test_sm3_on_every_fixture_length(engine):
    recs = fixture()["sm3"]
    msgs, want = [bytes.fromhex(r["msg"]) for r in recs], [int(r["digest"], 16) for r in recs]
    assert want[0] == int(model.SM3_ABC, 16) and want[1] == int(model.SM3_ABCD16, 16)
    for offset in (0, 1):                                                  # one length per lane, rows with garbage behind the message; word loads and byte loads
        view, lens = rows(engine, msgs, offset=offset)
        assert ints(engine.sm3(view, lens=lens)) == want, offset
        view, lens = rows(engine, msgs, width=203, offset=offset, garbage=0x80)
        assert ints(engine.sm3(view, lens=lens)) == want, offset
    for m, w in zip(msgs, want):                                           # equal lengths: a batch of 3 whose rows are a column slice of a wider array
        for offset in (0, 1):
            view, _ = rows(engine, [m + b"tail"] * 3, offset=offset)
            got = ints(engine.sm3(view[:, :len(m)]))
            assert got == [w] * 3, (len(m), offset)


def test_sm3_batch_sizes_against_the_model(engine):
    import random
    rng = random.Random(5)
    for n in SIZES:
        msgs = [bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 130)))) for _ in range(n)]
        view, lens = rows(engine, msgs, width=131, offset=1)
        assert ints(engine.sm3(view, lens=lens)) == [int(model.sm3(m).hex(), 16) for m in msgs], n


# ---- Z_A and e
def test_za_and_digest_on_every_fixture_record(engine):
    recs = message_records()
    for il in model.ID_LENGTHS:                                            # id_bytes is one value per call: the records of one identity length are one batch
        group = [m for m in recs if len(m["id"]) == il]
        assert len(group) == 12
        qx, qy = dev(engine, [m["q"][0] for m in group]), dev(engine, [m["q"][1] for m in group])
        msgs, lens = rows(engine, [m["msg"] for m in group], offset=1)
        if il:
            ids, _ = rows(engine, [m["id"] for m in group], offset=1)
            assert ints(engine.sm2_za(curve(), qx, qy, ids=ids)) == [m["za"] for m in group], il           # one identity per lane
            assert ints(engine.sm2_digest(curve(), qx, qy, msgs, ids=ids, lens=lens)) == [m["e"] for m in group], il
        shared = group[0]["id"]                                            # one identity for the whole batch
        assert ints(engine.sm2_za(curve(), qx, qy, ids=shared)) == [int(model.za(m["q"], shared).hex(), 16) for m in group], il
        assert ints(engine.sm2_digest(curve(), qx, qy, msgs, ids=shared, lens=lens)) == [model.digest(m["q"], shared, m["msg"]) for m in group], il
    for ml in model.MSG_LENGTHS:                                           # equal message lengths, word loads
        group = [m for m in recs if len(m["msg"]) == ml and len(m["id"]) == 16]
        qx, qy = dev(engine, [m["q"][0] for m in group]), dev(engine, [m["q"][1] for m in group])
        msgs, _ = rows(engine, [m["msg"] for m in group], width=max(ml, 1))
        want = [model.digest(m["q"], model.DEFAULT_ID, m["msg"]) for m in group]
        assert ints(engine.sm2_digest(curve(), qx, qy, msgs[:, :ml])) == want, ml
    ex = fixture()["example"]
    qx, qy = dev(engine, [I(ex, "qx")]), dev(engine, [I(ex, "qy")])
    assert ints(engine.sm2_za(curve(), qx, qy)) == [I(ex, "za")]
    msgs, _ = rows(engine, [bytes.fromhex(ex["msg"])])
    assert ints(engine.sm2_digest(curve(), qx, qy, msgs)) == [I(ex, "e")] == [model.EXAMPLE["e"]]
    long_id = bytes(range(256)) * 32
    for n_id in (8191, 1000, 127):
        assert ints(engine.sm2_za(curve(), qx, qy, ids=long_id[:n_id])) == [int(model.za((I(ex, "qx"), I(ex, "qy")), long_id[:n_id]).hex(), 16)], n_id


# ---- the fixture, bit for bit
def test_the_fixture_through_verify(engine):
    recs = message_records()
    for il in model.ID_LENGTHS:
        group = [m for m in recs if len(m["id"]) == il]
        qx, qy = dev(engine, [m["q"][0] for m in group]), dev(engine, [m["q"][1] for m in group])
        r, s = dev(engine, [m["r"] for m in group]), dev(engine, [m["s"] for m in group])
        msgs, lens = rows(engine, [m["msg"] for m in group], offset=1)
        ids = rows(engine, [m["id"] for m in group], offset=1)[0] if il else b""
        want = [m["ok"] for m in group]
        assert set(want) == {0, 1}
        assert flags(engine.sm2_verify(curve(), qx, qy, msgs, r, s, ids=ids, lens=lens)) == want, il
        e = engine.sm2_digest(curve(), qx, qy, msgs, ids=ids, lens=lens)                                 # verify equals digest -> verify_digest
        assert flags(engine.sm2_verify_digest(curve(), e, r, s, qx, qy)) == want, il


def test_verdicts_lane_by_lane_in_one_batch_that_mixes_every_record_kind(engine):
    lanes = digest_lanes()
    want = [l[4] for l in lanes]
    assert want.count(1) > 40 and want.count(0) > 40
    col = lambda f: dev(engine, [f(l) for l in lanes])
    qx, qy, e, r, s = col(lambda l: l[0][0]), col(lambda l: l[0][1]), col(lambda l: l[1]), col(lambda l: l[2]), col(lambda l: l[3])
    assert flags(engine.sm2_verify_digest(curve(), e, r, s, qx, qy)) == want
    back = lanes[::-1]                                                     # the same lanes in another order: a lane's verdict is its own
    col = lambda f: dev(engine, [f(l) for l in back])
    got = engine.sm2_verify_digest(curve(), col(lambda l: l[1]), col(lambda l: l[2]), col(lambda l: l[3]), col(lambda l: l[0][0]), col(lambda l: l[0][1]))
    assert flags(got) == want[::-1]
    fx = fixture()["digest"]                                               # and every digest-level record alone
    for rec in fx:
        one = engine.sm2_verify_digest(curve(), dev(engine, [I(rec, "e")]), dev(engine, [I(rec, "r")]), dev(engine, [I(rec, "s")]), dev(engine, [I(rec, "qx")]), dev(engine, [I(rec, "qy")]))
        assert flags(one) == [rec["ok"]], rec["note"]


def test_the_fixture_through_sign_digest_and_pubkey(engine):
    for det in (False, True):
        pool = sign_pool(det)
        assert {p[5] for p in pool} == {0, 1}
        e, d = dev(engine, [p[0] for p in pool]), dev(engine, [p[1] for p in pool])
        k = None if det else dev(engine, [p[2] for p in pool])
        r, s, ok = engine.sm2_sign_digest(curve(), e, d, k)
        assert flags(ok) == [p[5] for p in pool] and ints(r) == [p[3] for p in pool] and ints(s) == [p[4] for p in pool], det
        if det:                                                            # what the file stores for the deterministic records is what the model says now
            stored = [(I(x, "r"), I(x, "s"), x["ok"]) for x in fixture()["sign"] if x["k"] is None]
            assert stored == [p[3:] for p, x in zip(pool, fixture()["sign"]) if x["k"] is None]
        keys = pool                                                        # verify_digest accepts what sign_digest made, on the same lanes
        qx, qy, key_ok = engine.sm2_pubkey(curve(), d)
        assert flags(engine.sm2_verify_digest(curve(), e, r, s, qx, qy)) == [p[5] for p in keys], det
    keys = key_pool()
    qx, qy, ok = engine.sm2_pubkey(curve(), dev(engine, [k[0] for k in keys]))
    assert flags(ok) == [k[3] for k in keys] and {k[3] for k in keys} == {0, 1}
    assert ints(qx) == [k[1] for k in keys] and ints(qy) == [k[2] for k in keys]


def test_the_message_level_chain_signs_what_verify_accepts(engine):
    recs = [m for m in message_records() if len(m["id"]) == 16 and m["ok"] == 1]
    pool = [p for p in sign_pool(False) if 1 <= p[1] <= N - 2][:len(recs)]
    d, k = [p[1] for p in pool], [p[2] for p in pool]
    msgs, lens = rows(engine, [m["msg"] for m in recs[:len(pool)]], offset=1)
    ids, _ = rows(engine, [m["id"] for m in recs[:len(pool)]])
    for nonce in (dev(engine, k), None):
        r, s, ok, qx, qy = engine.sm2_sign(curve(), dev(engine, d), msgs, ids=ids, k=nonce, lens=lens)
        want = [model.sign(m["id"], m["msg"], dd, kk if nonce is not None else None) for m, dd, kk in zip(recs, d, k)]
        assert list(zip(ints(r), ints(s), flags(ok))) == want
        assert flags(engine.sm2_verify(curve(), qx, qy, msgs, r, s, ids=ids, lens=lens)) == [w[2] for w in want]


# ---- batch sizes
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(engine, n):
    lanes = tile(digest_lanes(), n)
    col = lambda f: dev(engine, [f(l) for l in lanes])
    got = engine.sm2_verify_digest(curve(), col(lambda l: l[1]), col(lambda l: l[2]), col(lambda l: l[3]), col(lambda l: l[0][0]), col(lambda l: l[0][1]))
    assert flags(got) == [l[4] for l in lanes]
    group = tile([m for m in message_records() if len(m["id"]) == 53], n)
    msgs, lens = rows(engine, [m["msg"] for m in group], width=101, offset=1)
    ids, _ = rows(engine, [m["id"] for m in group], width=53)
    qx, qy = dev(engine, [m["q"][0] for m in group]), dev(engine, [m["q"][1] for m in group])
    got = engine.sm2_verify(curve(), qx, qy, msgs, dev(engine, [m["r"] for m in group]), dev(engine, [m["s"] for m in group]), ids=ids, lens=lens)
    assert flags(got) == [m["ok"] for m in group]
    for det in (False, True):
        pool = tile(sign_pool(det), n)
        k = None if det else dev(engine, [p[2] for p in pool])
        r, s, ok = engine.sm2_sign_digest(curve(), dev(engine, [p[0] for p in pool]), dev(engine, [p[1] for p in pool]), k)
        assert flags(ok) == [p[5] for p in pool] and ints(r) == [p[3] for p in pool] and ints(s) == [p[4] for p in pool], det
    keys = tile(key_pool(), n)
    qx, qy, ok = engine.sm2_pubkey(curve(), dev(engine, [k[0] for k in keys]))
    assert flags(ok) == [k[3] for k in keys] and ints(qx) == [k[1] for k in keys] and ints(qy) == [k[2] for k in keys]


@pytest.mark.parametrize("det", [False, True])
def test_signing_where_a_lane_of_the_shared_inversion_holds_two_elements(engine, det):
    """2^18 + 1 signatures: m = 2, 131 073 lanes, the last with a single element.  Tiled from the signing records (good and refused keys and nonces side by
    side in one lane's running product); every lane is compared."""
    import torch
    n = TWO_PER_LANE
    pool = sign_pool(det)
    lanes = (n + 1) // 2
    assert len(pool) <= 256 and (n >> 17) == 2 and ((1 << 18) - 1) >> 17 == 1 and (lanes - 1) + lanes >= n > lanes        # m = 2 from 2^18 on; odd n: the last lane has one element
    idx = np.arange(n) % len(pool)
    idx[n // 2], idx[-1] = 3, 5                                             # element 2^17 is the last lane's only one; the batch's last element is its neighbour's second
    col = lambda j: limbs([p[j] for p in pool])[idx]
    on = lambda a: engine.to_device(a)
    r, s, ok = engine.sm2_sign_digest(curve(), on(col(0)), on(col(1)), None if det else on(col(2)))
    assert np.array_equal(ok.cpu().numpy(), np.array([p[5] for p in pool], dtype=np.uint8)[idx])
    assert np.array_equal(r.cpu().numpy().view(np.uint64), col(3)) and np.array_equal(s.cpu().numpy().view(np.uint64), col(4))
    if not det:
        keys = key_pool()
        kidx = np.arange(n) % len(keys)
        qx, qy, kok = engine.sm2_pubkey(curve(), on(limbs([k[0] for k in keys])[kidx]))
        assert np.array_equal(kok.cpu().numpy(), np.array([k[3] for k in keys], dtype=np.uint8)[kidx])
        assert np.array_equal(qx.cpu().numpy().view(np.uint64), limbs([k[1] for k in keys])[kidx]) and np.array_equal(qy.cpu().numpy().view(np.uint64), limbs([k[2] for k in keys])[kidx])
    torch.cuda.synchronize()


# ---- refusals
def test_refused_arguments_through_their_return_codes(engine):
    import torch
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    lib, ctx, null, cv = engine.lib, engine.ctx, C.c_void_p(0), C.c_int(curve())
    p = lambda t: C.c_void_p(t.data_ptr())
    z = lambda n=4: torch.zeros((n, 4), dtype=torch.int64, device=engine.tdev)
    a, b, c, d, e, out1, out2 = z(), z(), z(), z(), z(), z(), z()
    ok = torch.zeros(4, dtype=torch.uint8, device=engine.tdev)
    msg = torch.zeros((4, 8), dtype=torch.uint8, device=engine.tdev)
    ident = torch.zeros(8192, dtype=torch.uint8, device=engine.tdev)
    four, zero, s8 = C.c_size_t(4), C.c_size_t(0), C.c_size_t(8)
    sz = C.c_size_t
    err = lambda: lib.ecsimd_hip_last_error(ctx).decode()
    # null pointers with n > 0
    assert lib.ecsimd_sm2_sm3(ctx, null, s8, s8, null, p(out1), four) == -1 and lib.ecsimd_sm2_sm3(ctx, p(msg), s8, s8, null, null, four) == -1
    assert lib.ecsimd_sm2_za(ctx, cv, null, p(b), p(ident), sz(16), zero, p(out1), four) == -1 and lib.ecsimd_sm2_za(ctx, cv, p(a), p(b), null, sz(16), zero, p(out1), four) == -1
    assert lib.ecsimd_sm2_digest(ctx, cv, p(a), p(b), p(ident), sz(16), zero, null, s8, s8, null, p(out1), four) == -1
    assert lib.ecsimd_sm2_pubkey(ctx, cv, null, p(out1), p(out2), p(ok), four) == -1 and lib.ecsimd_sm2_pubkey(ctx, cv, p(a), p(out1), p(out2), null, four) == -1
    assert lib.ecsimd_sm2_verify_digest(ctx, cv, p(a), p(b), null, p(c), p(d), p(ok), four) == -1 and lib.ecsimd_sm2_verify_digest(ctx, cv, p(a), p(b), p(c), p(d), p(e), null, four) == -1
    assert lib.ecsimd_sm2_verify(ctx, cv, p(a), p(b), p(ident), sz(16), zero, p(msg), s8, s8, null, null, p(c), p(ok), four) == -1
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), null, p(c), p(out1), p(out2), p(ok), four, C.c_int(0)) == -1
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), p(b), null, p(out1), null, p(ok), four, C.c_int(0)) == -1
    assert lib.ecsimd_sm2_sign_digest(None, cv, p(a), p(b), p(c), p(out1), p(out2), p(ok), four, C.c_int(0)) == -1
    # outputs that are inputs or each other
    assert lib.ecsimd_sm2_za(ctx, cv, p(a), p(b), p(ident), sz(16), zero, p(a), four) == -1 and "alias" in err()
    assert lib.ecsimd_sm2_pubkey(ctx, cv, p(a), p(a), p(out2), p(ok), four) == -1 and lib.ecsimd_sm2_pubkey(ctx, cv, p(a), p(out1), p(out1), p(ok), four) == -1
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), p(b), p(c), p(a), p(out2), p(ok), four, C.c_int(0)) == -1
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), p(b), p(c), p(out1), p(out1), p(ok), four, C.c_int(0)) == -1 and "alias" in err()
    # the identity's length, flags, strides
    assert lib.ecsimd_sm2_za(ctx, cv, p(a), p(b), p(ident), sz(8192), zero, p(out1), four) == -1 and "8191" in err()
    assert lib.ecsimd_sm2_digest(ctx, cv, p(a), p(b), p(ident), sz(8192), zero, p(msg), s8, s8, null, p(out1), four) == -1
    assert lib.ecsimd_sm2_verify(ctx, cv, p(a), p(b), p(ident), sz(8192), zero, p(msg), s8, s8, null, p(c), p(d), p(ok), four) == -1
    assert lib.ecsimd_sm2_za(ctx, cv, p(a), p(b), p(ident), sz(8191), zero, p(out1), four) == 0
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), p(b), p(c), p(out1), p(out2), p(ok), four, C.c_int(1)) == -1 and "flags must be 0" in err()
    assert lib.ecsimd_sm2_sm3(ctx, p(msg), s8, sz(7), null, p(out1), four) == -1 and "stride_bytes is smaller" in err()
    assert lib.ecsimd_sm2_za(ctx, cv, p(a), p(b), p(ident), sz(16), sz(15), p(out1), four) == -1
    with pytest.raises(EcsimdHipError, match="flags must be 0"):
        engine.sm2_sign_digest(curve(), a, b, c, flags=2)
    # the built-in curve ids, an unknown id
    for bad in (0, 1, 9999):
        bc = C.c_int(bad)
        assert lib.ecsimd_sm2_za(ctx, bc, p(a), p(b), p(ident), sz(16), zero, p(out1), four) == -1
        assert ("built-in" in err()) == (bad < 2)
        assert lib.ecsimd_sm2_digest(ctx, bc, p(a), p(b), p(ident), sz(16), zero, p(msg), s8, s8, null, p(out1), four) == -1
        assert lib.ecsimd_sm2_pubkey(ctx, bc, p(a), p(out1), p(out2), p(ok), four) == -1
        assert lib.ecsimd_sm2_verify_digest(ctx, bc, p(a), p(b), p(c), p(d), p(e), p(ok), four) == -1
        assert lib.ecsimd_sm2_verify(ctx, bc, p(a), p(b), p(ident), sz(16), zero, p(msg), s8, s8, null, p(c), p(d), p(ok), four) == -1
        assert lib.ecsimd_sm2_sign_digest(ctx, bc, p(a), p(b), p(c), p(out1), p(out2), p(ok), four, C.c_int(0)) == -1
        assert lib.ecsimd_sm2_sign_digest(ctx, bc, p(a), p(b), null, p(out1), p(out2), p(ok), four, C.c_int(0)) == -1
    # more than 2^22 secret scalars in one call (refused before anything is touched: the arrays are too short on purpose)
    many = C.c_size_t((1 << 22) + 1)
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, p(a), p(b), p(c), p(out1), p(out2), p(ok), many, C.c_int(0)) == -1 and "2^22" in err()
    assert lib.ecsimd_sm2_pubkey(ctx, cv, p(a), p(out1), p(out2), p(ok), many) == -1 and "2^22" in err()
    # n = 0 is fine, with null pointers too
    assert lib.ecsimd_sm2_sm3(ctx, null, zero, zero, null, null, zero) == 0 and lib.ecsimd_sm2_za(ctx, cv, null, null, null, sz(16), zero, null, zero) == 0
    assert lib.ecsimd_sm2_pubkey(ctx, cv, null, null, null, null, zero) == 0 and lib.ecsimd_sm2_verify_digest(ctx, cv, null, null, null, null, null, null, zero) == 0
    assert lib.ecsimd_sm2_sign_digest(ctx, cv, null, null, null, null, null, null, zero, C.c_int(0)) == 0
    # a context that asks for the reference's squaring is refused as ECDSA refuses it
    eng = Engine(0)
    try:
        eng.set_ref_square_compat(True)
        x = lambda: torch.zeros((4, 4), dtype=torch.int64, device=eng.tdev)
        for call in (lambda: eng.sm2_za(curve(), x(), x()), lambda: eng.sm2_pubkey(curve(), x()), lambda: eng.sm2_verify_digest(curve(), x(), x(), x(), x(), x()),
                     lambda: eng.sm2_sign_digest(curve(), x(), x(), x()), lambda: eng.sm2_sign_digest(curve(), x(), x())):
            with pytest.raises(EcsimdHipError, match="REF_SQUARE_COMPAT"):
                call()
    finally:
        eng.close()


# ---- the workspace after the secret calls
@pytest.mark.parametrize("call", ["sign", "sign_deterministic", "pubkey"])
def test_the_used_prefix_of_the_workspace_is_zero_afterwards(call):
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    try:
        n = 200
        pool = tile(sign_pool(call == "sign_deterministic"), n)
        e, d = dev(eng, [p[0] for p in pool]), dev(eng, [p[1] for p in pool])
        k = dev(eng, [p[2] for p in pool]) if call == "sign" else None
        run = (lambda: eng.sm2_pubkey(curve(), d)) if call == "pubkey" else (lambda: eng.sm2_sign_digest(curve(), e, d, k))
        run(); torch.cuda.synchronize()
        ptr, size = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        flag_bytes = (n + 15) // 16 * 16
        used = 9 * 32 * n + 2 * flag_bytes                                           # the product's arrays: two adjusted scalars, the Jacobian point, two affine points, two flag arrays
        if call == "sign_deterministic":
            used += 32 * n + 96 * n + 2 * flag_bytes                                 # the nonce, K and V, the retry bytes and a byte array nobody reads
        assert ptr.value and size.value >= used
        fill = np.full(size.value, 0xA5, dtype=np.uint8)
        eng._bind_stream()
        eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(size.value)), "memcpy_h2d")
        got = run(); torch.cuda.synchronize()
        if call == "pubkey":
            assert ints(got[0]) == [model.pubkey(p[1])[0][0] for p in pool]
        else:
            assert ints(got[0]) == [p[3] for p in pool] and flags(got[2]) == [p[5] for p in pool]
        back = np.empty(size.value, dtype=np.uint8)
        eng._check(eng.lib.ecsimd_hip_memcpy_d2h(eng.ctx, back.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(size.value)), "memcpy_d2h")
        assert not back[:used].any(), np.flatnonzero(back[:used])[:8]
        assert (back[used:] == 0xA5).all()                                           # ... and nothing behind it was touched
    finally:
        eng.close()


# ---- graph capture: a fresh context, so that the first call under capture is the one that would have to grow the workspace
def test_capture_is_refused_before_the_warm_up_and_replays_after_it():
    import torch
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    n = 130
    recs = [m for m in message_records() if len(m["id"]) == 54]
    det, caller, keys = sign_pool(True), sign_pool(False), key_pool()

    def make(shift):
        g = [recs[(i + shift) % len(recs)] for i in range(n)]
        sd, sc, kk = ([p[(i + 5 * shift) % len(p)] for i in range(n)] for p in (det, caller, keys))
        return dict(group=g, det=sd, caller=sc, keys=kk)
    sets = [make(s) for s in range(3)]
    eng = Engine(0)
    try:
        def load(i, b=None):
            s = sets[i]
            t = dict(qx=dev(eng, [m["q"][0] for m in s["group"]]), qy=dev(eng, [m["q"][1] for m in s["group"]]), r=dev(eng, [m["r"] for m in s["group"]]),
                     s=dev(eng, [m["s"] for m in s["group"]]), e=dev(eng, [m["e"] for m in s["group"]]), msgs=rows(eng, [m["msg"] for m in s["group"]], width=100)[0],
                     lens=rows(eng, [m["msg"] for m in s["group"]], width=100)[1], ids=rows(eng, [m["id"] for m in s["group"]], width=54)[0],
                     de=dev(eng, [p[0] for p in s["det"]]), dd=dev(eng, [p[1] for p in s["det"]]), ce=dev(eng, [p[0] for p in s["caller"]]), cd=dev(eng, [p[1] for p in s["caller"]]),
                     ck=dev(eng, [p[2] for p in s["caller"]]), kd=dev(eng, [k[0] for k in s["keys"]]))
            if b is None:
                return t
            for k in t:
                b[k].copy_(t[k])
            return b

        def run(b):
            return dict(sm3=eng.sm3(b["msgs"], lens=b["lens"]), e=eng.sm2_digest(curve(), b["qx"], b["qy"], b["msgs"], ids=b["ids"], lens=b["lens"]),
                        v=eng.sm2_verify(curve(), b["qx"], b["qy"], b["msgs"], b["r"], b["s"], ids=b["ids"], lens=b["lens"]),
                        vd=eng.sm2_verify_digest(curve(), b["e"], b["r"], b["s"], b["qx"], b["qy"]), det=eng.sm2_sign_digest(curve(), b["de"], b["dd"]),
                        caller=eng.sm2_sign_digest(curve(), b["ce"], b["cd"], b["ck"]), pub=eng.sm2_pubkey(curve(), b["kd"]))

        bufs = load(0)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        said = {}
        with torch.cuda.stream(side):
            with torch.cuda.graph(g0, stream=side):
                for name, call in (("verify", lambda: eng.sm2_verify(curve(), bufs["qx"], bufs["qy"], bufs["msgs"], bufs["r"], bufs["s"], ids=bufs["ids"], lens=bufs["lens"])),
                                   ("verify_digest", lambda: eng.sm2_verify_digest(curve(), bufs["e"], bufs["r"], bufs["s"], bufs["qx"], bufs["qy"])),
                                   ("sign", lambda: eng.sm2_sign_digest(curve(), bufs["ce"], bufs["cd"], bufs["ck"])),
                                   ("sign_deterministic", lambda: eng.sm2_sign_digest(curve(), bufs["de"], bufs["dd"])), ("pubkey", lambda: eng.sm2_pubkey(curve(), bufs["kd"]))):
                    try:
                        call(); said[name] = "it did not refuse"
                    except EcsimdHipError as e:
                        said[name] = str(e)
                marker = bufs["e"] + 1                                               # the capture is still valid: this node is recorded
        torch.cuda.synchronize()
        for name, text in said.items():
            assert "(-1)" in text and "the context workspace would have to grow during stream capture" in text, (name, text)
        g0.replay(); torch.cuda.synchronize()
        assert torch.equal(marker, bufs["e"] + 1)
        del g0
        run(bufs); torch.cuda.synchronize()                                          # the warm-up at the capture's batch size and lengths
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out = run(bufs)
        torch.cuda.synchronize()
        for i in (1, 2):
            load(i, bufs); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            s = sets[i]
            assert ints(out["sm3"]) == [int(model.sm3(m["msg"]).hex(), 16) for m in s["group"]] and ints(out["e"]) == [m["e"] for m in s["group"]], i
            assert flags(out["v"]) == [m["ok"] for m in s["group"]] == flags(out["vd"]), i
            for key in ("det", "caller"):
                r, sg, ok = out[key]
                assert list(zip(ints(r), ints(sg), flags(ok))) == [p[3:] for p in s[key]], (i, key)
            qx, qy, ok = out["pub"]
            assert list(zip(ints(qx), ints(qy), flags(ok))) == [k[1:] for k in s["keys"]], i
        del g
    finally:
        eng.close()
