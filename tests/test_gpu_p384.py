"""GPU suite for NIST P-384 (include/ecsimd_p384.h).  Every expected value comes from tools/p384_model.py (Python integers, hashlib, hmac) or from
tests/golden/p384_vectors.json (RFC 6979 A.2.6 and records adjudicated by libcrypto when the file was minted), never from the library.  Layer by layer
through ecsimd_p384_raw -- the field and the scalars against Python integers on operands built for the longest carry and borrow runs, the complete group law on
its exceptional pairs, the three window loops on the scalars that reach the signed recoding's carries -- then the five calls: the fixture bit for bit, the
verdicts (x(R) >= n among them), signing against the model, ECDH both ways, SHA-384 on the padding boundaries, unaligned arrays, the chunk boundary, graph
replay and the wiped workspace."""
import ctypes as C
import functools
import hashlib
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import p384_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
P, N, G = model.P, model.N, model.G
i2b, b2i = model.i2b, model.b2i
OP = dict(FE_MUL=0, FE_SQR=1, FE_ADD=2, FE_SUB=3, FE_NEG=4, FE_INVERT=5, FE_CANON=6, SC_MUL=7, SC_INVERT=8, DECODE_ENCODE=9, POINT_ADD=10, POINT_DBL=11, BASE_MULT=12,
          VAR_MULT=13, DOUBLE_MULT=14)
CHUNK = 1 << 16
ALL = 2**384 - 1
ZERO, ONE = bytes(48), i2b(1)


def dev_rows(engine, rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    return torch.from_numpy(a).to(engine.tdev)


def at_offset(engine, rows, width, offset=1):
    """rows as an (n, width) device view `offset` bytes into its allocation"""
    import torch
    n = len(rows)
    buf = torch.zeros(width * n + 8, dtype=torch.uint8, device=engine.tdev)
    view = buf[offset:offset + width * n].view(n, width)
    view.copy_(dev_rows(engine, rows, width))
    assert view.data_ptr() % 4 == offset % 4
    return view


def host_rows(t):
    return [bytes(r) for r in t.cpu().numpy()]


def raw(engine, op, *columns):
    """ecsimd_p384_raw on columns of integers; returns the output records per lane as integers."""
    n = len(columns[0])
    rec = [b"".join(i2b(c[i]) for c in columns) for i in range(n)]
    out = host_rows(engine.p384_raw(OP[op], dev_rows(engine, rec, 48 * len(columns))))
    return [[b2i(o[k:k + 48]) for k in range(0, len(o), 48)] for o in out]


def point_out(pt):
    return [0, 0, 1] if pt is None else [pt[0], pt[1], 0]


def operands():
    """The constructed operands of the issue: the neighbours of 0, p and 2^384, one word all ones and its complement, 2^(32 j) +- 1."""
    ops = [0, 1, 2, P - 2, P - 1, P, P + 1, ALL]
    ops += [0xffffffff << (32 * j) for j in range(12)] + [ALL ^ (0xffffffff << (32 * j)) for j in range(12)]
    ops += [2**(32 * j) + s for j in range(1, 12) for s in (1, -1)]
    return ops


def operand_pairs(mod):
    rng = random.Random(384)
    ops = operands() + [N - 1, N, N + 1]
    pairs = [(a, a) for a in ops] + [(a, ops[(i * 7 + 3) % len(ops)]) for i, a in enumerate(ops)]
    pairs += [(P - 1, P - 1), (N - 1, N - 1), (ALL, ALL), (ALL, 1), (1, ALL)]
    # "the product's high half is all ones" cannot happen for two 384-bit factors: (2^384 - 1)^2 = 2^768 - 2^385 + 1 has the largest high half there is,
    # 2^384 - 2.  The pairs around it stand for the case: the high half's words are all ones but the lowest.
    pairs += [(ALL, ALL - 1), (ALL - 1, ALL - 1), (ALL, 2**383), (ALL, ALL ^ 0xffffffff)]
    pairs += [(rng.getrandbits(384), rng.getrandbits(384)) for _ in range(200)]
    return pairs


# ---- the field and the scalars
def test_field_operations_equal_python_integers(engine):
    pairs = operand_pairs(P)
    assert len(pairs) >= 65
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    for op, fn in (("FE_MUL", lambda x, y: x * y), ("FE_ADD", lambda x, y: x + y), ("FE_SUB", lambda x, y: x - y)):
        got = raw(engine, op, a, b)
        assert [g[0] for g in got] == [fn(x, y) % P for x, y in pairs], op
    for op, fn in (("FE_SQR", lambda x: x * x), ("FE_NEG", lambda x: -x), ("FE_CANON", lambda x: x)):
        got = raw(engine, op, a + b)
        assert [g[0] for g in got] == [fn(x) % P for x in a + b], op


def test_field_inversion(engine):
    vals = operands() + [random.Random(5).getrandbits(384) for _ in range(64)]
    got = [g[0] for g in raw(engine, "FE_INVERT", vals)]
    for v, inv in zip(vals, got):
        assert inv < P and (v * inv) % P == (0 if v % P == 0 else 1), hex(v)
    assert got[0] == 0 and got[5] == 0                                              # 0 and p: 0 -> 0


def test_scalar_product_and_inversion_modulo_n(engine):
    pairs = operand_pairs(N)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    assert [g[0] for g in raw(engine, "SC_MUL", a, b)] == [x * y % N for x, y in pairs]
    vals = operands() + [N - 1, N, N + 1] + [random.Random(6).getrandbits(384) for _ in range(64)]
    got = [g[0] for g in raw(engine, "SC_INVERT", vals)]
    for v, inv in zip(vals, got):
        assert inv < N and (v * inv) % N == (0 if v % N == 0 else 1), hex(v)


# ---- the group law
@functools.lru_cache(maxsize=None)
def some_points():
    rng = random.Random(4)
    return tuple(model.mult(rng.randrange(1, N)) for _ in range(4))


def test_the_complete_addition_on_every_kind_of_pair(engine):
    p, q = some_points()[:2]
    cases = [(p, q), (p, p), (p, model.neg(p)), (None, p), (p, None), (None, None), (G, G), (G, model.neg(G)), (q, p)]
    cols = [[], [], [], [], [], []]
    for a, b in cases:
        for col, v in zip(cols, point_out(a) + point_out(b)):
            col.append(v)
    # an identity operand's coordinates are ignored: hand over garbage there
    cols[0][3], cols[1][3] = 5, 7
    got = raw(engine, "POINT_ADD", *cols)
    assert got == [point_out(model.add(a, b)) for a, b in cases]
    dbl = raw(engine, "POINT_DBL", [p[0], G[0], 9], [p[1], G[1], 9], [0, 0, 1])
    assert dbl == [point_out(model.add(p, p)), point_out(model.add(G, G)), point_out(None)]
    assert dbl[0] == got[1] and dbl[1] == got[6]                                    # P + P by Algorithm 4 is the doubling of Algorithm 6


def test_decoding_validates(engine):
    p = some_points()[0]
    rows = [(p[0], p[1], 1), (G[0], G[1], 1), (P, p[1], 0), (p[0], P, 0), (p[0], (p[1] + 1) % P, 0), (0, 0, 0), (p[0], P - p[1], 1), (ALL, ALL, 0)]
    got = raw(engine, "DECODE_ENCODE", [r[0] for r in rows], [r[1] for r in rows])
    for r, g in zip(rows, got):
        assert g == ([r[0], r[1], 1] if r[2] else [0, 0, 0]), r


def window_scalars():
    rng = random.Random(16)
    ks = [0, 1, 2, 15, 16, N - 2, N - 1, N, N + 1, ALL]
    ks += [d << (4 * w) for w in range(96) for d in (8,)] + [rng.randrange(1, 16) << (4 * w) for w in range(96)]      # every window 0 but one
    ks += [int("8" * 96, 16), int("7" * 96, 16), int("f" * 96, 16), int("87" * 48, 16), int("78" * 48, 16)]
    ks += [rng.getrandbits(384) for _ in range(100)]
    return ks


@functools.lru_cache(maxsize=None)
def base_products():
    ks = window_scalars()
    return tuple(ks), tuple(model.mult(k) for k in ks)


def test_the_comb_against_the_model(engine):
    ks, want = base_products()
    got = raw(engine, "BASE_MULT", list(ks))
    assert got == [point_out(w) for w in want]


def test_the_variable_base_loop_against_the_model(engine):
    ks, want = base_products()
    n = len(ks)
    q = some_points()[2]
    for pt, exp in ((G, want), (model.neg(G), [model.neg(w) for w in want]), (q, None)):
        if exp is None:
            sub = list(ks[:10]) + list(ks[10:202:8]) + list(ks[202:207]) + list(ks[207:227])                     # the edges, a window in eight, the patterns, 20 random
            got = raw(engine, "VAR_MULT", sub, [pt[0]] * len(sub), [pt[1]] * len(sub))
            assert got == [point_out(model.mult(k, pt)) for k in sub]
        else:
            got = raw(engine, "VAR_MULT", list(ks), [pt[0]] * n, [pt[1]] * n)
            assert got == [point_out(w) for w in exp]


def test_the_double_product_of_verification(engine):
    rng = random.Random(8)
    q = some_points()[3]
    dq = 0x1234567                                                                   # a Q whose discrete logarithm is known: u1 G = -u2 Q can be arranged
    q2 = model.mult(dq)
    u = rng.randrange(1, N)
    cases = [(0, 5, q), (5, 0, q), (0, 0, q), (u, u, G), (u, N - u, G), (u * dq % N, N - u, q2), (N - 1, N - 1, q), (ALL, ALL, q)]
    cases += [(rng.getrandbits(384), rng.getrandbits(384), q) for _ in range(24)]
    got = raw(engine, "DOUBLE_MULT", [c[0] for c in cases], [c[1] for c in cases], [c[2][0] for c in cases], [c[2][1] for c in cases])
    want = [point_out(model.add(model.mult(u1), model.mult(u2, pt))) for u1, u2, pt in cases]
    assert got == want
    assert want[2] == want[4] == want[5] == [0, 0, 1] and want[3] == point_out(model.mult(2 * u))


# ---- the fixture
@functools.lru_cache(maxsize=None)
def fixture():
    return model.load_fixture()


def hexcol(recs, key):
    return [bytes.fromhex(r[key]) for r in recs]


def test_the_fixture_bit_for_bit_through_all_five_calls(engine):
    fx = fixture()
    pub, ok = engine.p384_pubkey(dev_rows(engine, hexcol(fx["base"], "k"), 48))
    assert host_rows(pub) == hexcol(fx["base"], "pub") and ok.cpu().tolist() == [1] * len(fx["base"])
    z, ok = engine.p384_ecdh(dev_rows(engine, hexcol(fx["ecdh"], "d"), 48), dev_rows(engine, hexcol(fx["ecdh"], "peer"), 96))
    assert host_rows(z) == hexcol(fx["ecdh"], "z") and ok.cpu().tolist() == [1] * len(fx["ecdh"])
    s = fx["sign"]
    assert bytes.fromhex(s[0]["msg"]) == b"sample" and bytes.fromhex(s[1]["msg"]) == b"test"
    assert s[0]["sig"].upper().startswith("94EDBB92A5ECB8AAD4736E56C691916B") and s[1]["sig"].upper().endswith("6A739F040649A667BF3B828246BAA5A5")     # RFC 6979 A.2.6
    msgs = hexcol(s, "msg")
    stride = (max(len(m) for m in msgs) + 3) // 4 * 4
    import torch
    lens = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=engine.tdev)
    digest = engine.p384_sha384(dev_rows(engine, [m + bytes(stride - len(m)) for m in msgs], stride), lens=lens)
    assert host_rows(digest) == hexcol(s, "digest")
    sig, ok = engine.p384_ecdsa_sign(dev_rows(engine, hexcol(s, "d"), 48), digest)
    assert host_rows(sig) == hexcol(s, "sig") and ok.cpu().tolist() == [1] * len(s)
    assert host_rows(engine.p384_pubkey(dev_rows(engine, hexcol(s, "d"), 48))[0]) == hexcol(s, "pub")
    v = fx["verify"]
    got = engine.p384_ecdsa_verify(dev_rows(engine, hexcol(v, "pub"), 96), dev_rows(engine, hexcol(v, "digest"), 48), dev_rows(engine, hexcol(v, "sig"), 96))
    wrong = [r["note"] for g, r in zip(got.cpu().tolist(), v) if g != r["ok"]]
    assert not wrong, wrong
    notes = {r["note"]: r["ok"] for r in v}
    for note, verdict in (("r = 0", 0), ("s = 0", 0), ("r = n", 0), ("s = n", 0), ("r = 2^384 - 1", 0), ("digest all ff (e >= n)", 1), ("digest = n (u1 = 0)", 1),
                          ("e = -r d (the sum is the identity)", 0), ("x(R) = n + 2, r = 2", 1), ("x(R) = n + 2, r = 3", 0), ("public key: x = p", 0),
                          ("public key: y = p", 0), ("public key: off the curve by one in y", 0), ("public key: (0, 0)", 0), ("public key: x + p", 0)):
        assert notes[note] == verdict, note


# ---- 257 distinct lanes from the model, shared by the tests below (and left unchanged)
@functools.lru_cache(maxsize=None)
def lanes():
    rng = random.Random(257)
    d = [i2b(rng.randrange(1, N)) for _ in range(257)]
    d[:4] = [i2b(1), i2b(2), i2b(N - 2), i2b(N - 1)]
    msgs = [bytes(rng.randrange(256) for _ in range(40)) for _ in range(257)]
    digest = [model.sha384(m) for m in msgs]
    digest[5], digest[6] = b"\xff" * 48, i2b(N)
    pub = [model.pubkey(x)[0] for x in d]
    sig = [model.sign(x, h)[0] for x, h in zip(d, digest)]
    peer = pub[1:] + pub[:1]
    z = [model.ecdh(x, q)[0] for x, q in zip(d, peer)]
    return dict(d=d, msgs=msgs, digest=digest, pub=pub, sig=sig, peer=peer, z=z)


def flip(b, bit):
    return bytes(v ^ (1 << (bit % 8)) if q == bit // 8 else v for q, v in enumerate(b))


def test_verdicts_on_valid_signatures_and_on_every_kind_of_one_bit_change(engine):
    L = lanes()
    n = 256
    rng = random.Random(1)
    pub, digest, sig = L["pub"][:n], L["digest"][:n], L["sig"][:n]
    run = lambda p, h, s: engine.p384_ecdsa_verify(dev_rows(engine, p, 96), dev_rows(engine, h, 48), dev_rows(engine, s, 96)).cpu().tolist()
    assert run(pub, digest, sig) == [1] * n
    assert run([flip(p, rng.randrange(768)) for p in pub], digest, sig) == [0] * n
    assert run(pub, [flip(h, rng.randrange(384)) for h in digest], sig) == [0] * n
    assert run(pub, digest, [flip(s, rng.randrange(384)) for s in sig]) == [0] * n          # r
    assert run(pub, digest, [flip(s, 384 + rng.randrange(384)) for s in sig]) == [0] * n    # s


def test_signing_equals_the_model_and_verifies(engine):
    L = lanes()
    n = 256
    d = L["d"][:n] + [ZERO, i2b(N), i2b(ALL)]
    digest = L["digest"][:n] + [L["digest"][0]] * 3
    dd, hd = dev_rows(engine, d, 48), dev_rows(engine, digest, 48)
    sig, ok = engine.p384_ecdsa_sign(dd, hd)
    assert host_rows(sig) == L["sig"][:n] + [bytes(96)] * 3
    assert ok.cpu().tolist() == [1] * n + [0] * 3
    pub, pok = engine.p384_pubkey(dd)
    assert host_rows(pub) == L["pub"][:n] + [bytes(96)] * 3 and pok.cpu().tolist() == [1] * n + [0] * 3
    assert engine.p384_ecdsa_verify(pub, hd, sig).cpu().tolist() == [1] * n + [0] * 3


def test_ecdh_both_ways_and_refusals(engine):
    L = lanes()
    n = 128
    d, peer = L["d"][:n], L["peer"][:n]
    z, ok = engine.p384_ecdh(dev_rows(engine, d, 48), dev_rows(engine, peer, 96))
    assert host_rows(z) == L["z"][:n] and ok.cpu().tolist() == [1] * n               # lanes 0 .. 3: d = 1, 2, n - 2, n - 1
    # the other side: lane i's peer is lane i + 1's key, so d[i + 1] on pub[i] agrees
    z2, ok2 = engine.p384_ecdh(dev_rows(engine, L["d"][1:n + 1], 48), dev_rows(engine, L["pub"][:n], 96))
    assert host_rows(z2) == L["z"][:n] and ok2.cpu().tolist() == [1] * n
    bad_peer = [peer[0][:48] + i2b((b2i(peer[0][48:]) + 1) % P), bytes(96), i2b(P) + peer[0][48:], peer[0], peer[0], peer[0]]
    bad_d = [d[5]] * 3 + [ZERO, i2b(N), d[5]]
    z3, ok3 = engine.p384_ecdh(dev_rows(engine, bad_d, 48), dev_rows(engine, bad_peer, 96))
    assert ok3.cpu().tolist() == [0, 0, 0, 0, 0, 1]
    assert host_rows(z3) == [ZERO] * 5 + [model.ecdh(d[5], peer[0])[0]]


# ---- SHA-384
SHA_LENGTHS = (0, 1, 111, 112, 127, 128, 129, 239, 240, 256)


def test_sha384_on_the_padding_boundaries(engine):
    import torch
    rng = random.Random(3)
    for length in SHA_LENGTHS:                                                       # equal lengths, at offset 0 and 1
        msgs = [bytes(rng.randrange(256) for _ in range(length)) for _ in range(5)]
        want = [hashlib.sha384(m).digest() for m in msgs]
        if length:
            assert host_rows(engine.p384_sha384(dev_rows(engine, msgs, length))) == want, length
            assert host_rows(engine.p384_sha384(at_offset(engine, msgs, length))) == want, length
        else:
            assert host_rows(engine.p384_sha384(torch.zeros((5, 0), dtype=torch.uint8, device=engine.tdev))) == want
    stride = 256
    msgs = [bytes(rng.randrange(256) for _ in range(length)) for length in SHA_LENGTHS * 7]
    lens = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=engine.tdev)
    want = [hashlib.sha384(m).digest() for m in msgs]
    padded = [m + b"\xa5" * (stride - len(m)) for m in msgs]
    assert host_rows(engine.p384_sha384(dev_rows(engine, padded, stride), lens=lens)) == want
    assert host_rows(engine.p384_sha384(at_offset(engine, padded, stride), lens=lens)) == want


# ---- batches
def tiled(col, n):
    return [col[i % 257] for i in range(n)]


def run_all(engine, L, n, place):
    """The five calls on n lanes tiled from the 257, every array placed by `place`; returns what they gave."""
    import torch
    d, digest, pub, sig, peer = (place(tiled(L[k], n), w) for k, w in (("d", 48), ("digest", 48), ("pub", 96), ("sig", 96), ("peer", 96)))
    msgs = place(tiled(L["msgs"], n), 40)
    out = dict(sha=engine.p384_sha384(msgs), pub=engine.p384_pubkey(d), z=engine.p384_ecdh(d, peer), ok=engine.p384_ecdsa_verify(pub, digest, sig),
               sig=engine.p384_ecdsa_sign(d, digest))
    torch.cuda.synchronize()
    return out


def check_all(out, L, n):
    assert host_rows(out["sha"]) == [hashlib.sha384(m).digest() for m in tiled(L["msgs"], n)]
    assert host_rows(out["pub"][0]) == tiled(L["pub"], n) and out["pub"][1].cpu().tolist() == [1] * n
    assert host_rows(out["z"][0]) == tiled(L["z"], n) and out["z"][1].cpu().tolist() == [1] * n
    assert out["ok"].cpu().tolist() == [1] * n
    assert host_rows(out["sig"][0]) == tiled(L["sig"], n) and out["sig"][1].cpu().tolist() == [1] * n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_batch_sizes_with_every_array_at_byte_offset_one(engine, n):
    L = lanes()
    check_all(run_all(engine, L, n, lambda rows, w: at_offset(engine, rows, w)), L, n)


def test_one_call_across_the_chunk_boundary(engine):
    L = lanes()
    n = CHUNK + 1
    import torch
    base = {k: dev_rows(engine, L[k], w) for k, w in (("d", 48), ("digest", 48), ("pub", 96), ("sig", 96), ("peer", 96), ("msgs", 40), ("z", 48))}
    idx = torch.arange(n, device=engine.tdev) % 257
    t = {k: v[idx].contiguous() for k, v in base.items()}
    bad = [CHUNK - 1, CHUNK]                                                         # a refused lane on either side of the boundary
    for b in bad:
        t["sig"][b, 95] ^= 1
    ok = engine.p384_ecdsa_verify(t["pub"], t["digest"], t["sig"])
    want = torch.ones(n, dtype=torch.uint8, device=engine.tdev); want[bad] = 0
    assert torch.equal(ok, want)
    for b in bad:
        t["sig"][b, 95] ^= 1
    pub, pok = engine.p384_pubkey(t["d"])
    assert torch.equal(pub, t["pub"]) and bool(pok.all())
    z, zok = engine.p384_ecdh(t["d"], t["peer"])
    assert torch.equal(z, t["z"]) and bool(zok.all())
    sig, sok = engine.p384_ecdsa_sign(t["d"], t["digest"])
    assert torch.equal(sig, t["sig"]) and bool(sok.all())
    sha = engine.p384_sha384(t["msgs"])
    assert host_rows(sha[CHUNK - 2:]) == [hashlib.sha384(L["msgs"][i % 257]).digest() for i in range(CHUNK - 2, n)]


def test_empty_batches_and_refused_arguments(engine):
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    e = lambda w: torch.zeros((0, w), dtype=torch.uint8, device=engine.tdev)
    assert engine.p384_sha384(e(7)).shape == (0, 48)
    assert engine.p384_pubkey(e(48))[0].shape == (0, 96)
    assert engine.p384_ecdh(e(48), e(96))[0].shape == (0, 48)
    assert engine.p384_ecdsa_verify(e(96), e(48), e(96)).shape == (0,)
    assert engine.p384_ecdsa_sign(e(48), e(48))[0].shape == (0, 96)
    assert engine.p384_raw(OP["FE_MUL"], e(96)).shape == (0, 48)
    L = lanes()
    d, h = dev_rows(engine, L["d"][:4], 48), dev_rows(engine, L["digest"][:4], 48)
    with pytest.raises(EcsimdHipError, match="flags must be 0"):
        engine.p384_ecdsa_sign(d, h, flags=1)
    with pytest.raises(EcsimdHipError, match="unknown function"):
        engine.p384_raw(15, d)
    lib, ctx, null = engine.lib, engine.ctx, C.c_void_p(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    out96, ok = torch.zeros((4, 96), dtype=torch.uint8, device=engine.tdev), torch.zeros(4, dtype=torch.uint8, device=engine.tdev)
    four = C.c_size_t(4)
    assert lib.ecsimd_p384_pubkey(ctx, null, p(out96), p(ok), four) == -1 and lib.ecsimd_p384_pubkey(ctx, p(d), p(out96), null, four) == -1
    assert lib.ecsimd_p384_ecdh(ctx, p(d), null, p(out96), p(ok), four) == -1
    assert lib.ecsimd_p384_ecdsa_verify(ctx, p(out96), p(h), null, p(ok), four) == -1
    assert lib.ecsimd_p384_ecdsa_sign(ctx, p(d), p(h), null, p(ok), four, C.c_int(0)) == -1
    assert lib.ecsimd_p384_sha384(ctx, null, C.c_size_t(8), C.c_size_t(8), null, p(out96), four) == -1
    assert lib.ecsimd_p384_pubkey(ctx, p(d), p(d), p(ok), four) == -1                # an output that is an input
    assert lib.ecsimd_p384_pubkey(None, p(d), p(out96), p(ok), four) == -1


# ---- graph capture: a fresh context, so that the first call under capture is the one that would have to grow the workspace
def test_capture_is_refused_before_the_warm_up_and_replays_after_it():
    import torch
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    L = lanes()
    n = 130
    sets = [{k: [L[k][(i + 40 * s) % 257] for i in range(n)] for k in ("d", "digest", "pub", "sig", "peer", "z", "msgs")} for s in range(3)]
    for s in sets:
        s["sig"] = [flip(g, 700) if j in (7, 64, 129) else g for j, g in enumerate(s["sig"])]
        s["ok"] = [int(j not in (7, 64, 129)) for j in range(n)]
    eng = Engine(0)
    try:
        widths = dict(d=48, digest=48, pub=96, sig=96, peer=96, msgs=40)

        def load(i, b=None):
            t = {k: dev_rows(eng, sets[i][k], w) for k, w in widths.items()}
            if b is None:
                return t
            for k in t:
                b[k].copy_(t[k])
            return b

        def run(b):
            return dict(sha=eng.p384_sha384(b["msgs"]), pub=eng.p384_pubkey(b["d"])[0], z=eng.p384_ecdh(b["d"], b["peer"])[0],
                        ok=eng.p384_ecdsa_verify(b["pub"], b["digest"], b["sig"]), sig=eng.p384_ecdsa_sign(b["d"], b["digest"])[0])

        bufs = load(0)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        said = {}
        with torch.cuda.stream(side):
            with torch.cuda.graph(g0, stream=side):
                for name, call in (("ecdh", lambda: eng.p384_ecdh(bufs["d"], bufs["peer"])), ("verify", lambda: eng.p384_ecdsa_verify(bufs["pub"], bufs["digest"], bufs["sig"])),
                                   ("sign", lambda: eng.p384_ecdsa_sign(bufs["d"], bufs["digest"]))):
                    try:
                        call(); said[name] = "it did not refuse"
                    except EcsimdHipError as e:
                        said[name] = str(e)
                marker = bufs["d"] + 1                                               # the capture is still valid: this node is recorded
        torch.cuda.synchronize()
        for name, text in said.items():
            assert "(-1)" in text and "the context workspace would have to grow during stream capture" in text, (name, text)
        g0.replay(); torch.cuda.synchronize()
        assert torch.equal(marker, bufs["d"] + 1)
        del g0
        run(bufs); torch.cuda.synchronize()                                          # the warm-up at the capture's batch size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out = run(bufs)
        torch.cuda.synchronize()
        for i in (1, 2):
            load(i, bufs); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            s = sets[i]
            assert host_rows(out["sha"]) == [hashlib.sha384(m).digest() for m in s["msgs"]], i
            assert host_rows(out["pub"]) == s["pub"] and host_rows(out["z"]) == s["z"], i
            assert out["ok"].cpu().tolist() == s["ok"], i
            assert host_rows(out["sig"]) == [L["sig"][(j + 40 * i) % 257] for j in range(n)], i
        del g
    finally:
        eng.close()


# ---- the workspace after the secret calls
@pytest.mark.parametrize("call", ["sign", "ecdh"])
def test_the_used_prefix_of_the_workspace_is_zero_afterwards(call):
    import torch
    from ecsimd_amd import Engine
    L = lanes()
    eng = Engine(0)
    try:
        n = 200
        d, h, peer = dev_rows(eng, L["d"][:n], 48), dev_rows(eng, L["digest"][:n], 48), dev_rows(eng, L["peer"][:n], 96)
        run = (lambda: eng.p384_ecdsa_sign(d, h)) if call == "sign" else (lambda: eng.p384_ecdh(d, peer))
        run(); torch.cuda.synchronize()
        ptr, size = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        used = n * (52 if call == "sign" else 1152)                                  # k and its validity: 13 words; the table: 8 x 36 words
        assert ptr.value and size.value >= used
        fill = np.full(size.value, 0xA5, dtype=np.uint8)
        eng._bind_stream()
        eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(size.value)), "memcpy_h2d")
        got = run(); torch.cuda.synchronize()
        assert host_rows(got[0]) == (L["sig"][:n] if call == "sign" else L["z"][:n])
        back = np.empty(size.value, dtype=np.uint8)
        eng._check(eng.lib.ecsimd_hip_memcpy_d2h(eng.ctx, back.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(size.value)), "memcpy_d2h")
        assert not back[:used].any(), np.flatnonzero(back[:used])[:8]
        assert (back[used:] == 0xA5).all()                                           # ... and nothing behind it was touched
    finally:
        eng.close()
