"""GPU suite for Ed25519 (include/ecsimd_ed25519.h).  Every expected value comes from tools/ed25519_model.py (plain Python integers, hashlib) or from
tests/golden/ed25519_vectors.json (RFC 8032 7.1 TEST 1-3 and records minted from libcrypto).  Layer by layer through ecsimd_ed25519_raw -- the field against
Python integers AND against Engine.mod_mul etc. on register_modulus(2^255 - 19), a second device path that shares no code with fe25519.cuh --, then the three
calls: the fixture bit for bit, the padding boundaries of both hashes, unaligned arrays, the chunk boundary, graph replay, and the wiped workspace.
tests/golden/ed25519_verdicts.json carries the verdict of every refused and accepted kind of lane as libcrypto and the model gave it when the file was minted
(tests/test_ed25519_cpu.py holds both to it): the tests that read it run no model on the host.  Points with a small-order component -- [k]B + T -- go
through every layer and through verification, where the cofactorless equation is decided by (h mod L) mod 8."""
import ctypes as C
import functools
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
P, L = model.P, model.L
OP = dict(MUL=0, SQR=1, ADD=2, SUB=3, NEG=4, INVERT=5, CANON=6, SQRT_RATIO=7, DECODE_ENCODE=8, POINT_ADD=9, POINT_DBL=10, SC_REDUCE=11, BASE_MULT=12, DOUBLE_MULT=13)
LENGTHS = (0, 1, 79, 80, 81, 95, 96, 97, 128, 207, 208, 300)
EDGE = (0, 1, 2, 19, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1, 2**256 - 38, 2**256 - 39)
ZERO32 = bytes(32)


def le32(v):
    return int(v).to_bytes(32, "little")


def dev_rows(engine, rows, width):
    """A list of byte strings of `width` bytes -> an (n, width) uint8 device tensor."""
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    return torch.from_numpy(a).to(engine.tdev)


def at_offset(engine, rows, width, offset):
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
    """ecsimd_ed25519_raw on columns of 32-byte strings; returns the list of output records per lane (each a list of 32-byte strings)."""
    n = len(columns[0])
    rec = [b"".join(c[i] for c in columns) for i in range(n)]
    out = host_rows(engine.ed25519_raw(OP[op], dev_rows(engine, rec, 32 * len(columns))))
    return [[o[k:k + 32] for k in range(0, len(o), 32)] for o in out]


@functools.lru_cache(maxsize=None)
def fixture():
    return tuple((bytes.fromhex(c["seed"]), bytes.fromhex(c["message"]), bytes.fromhex(c["public_key"]), bytes.fromhex(c["signature"]))
                 for c in json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json")))["cases"])


@functools.lru_cache(maxsize=None)
def model_sign(seed, msg):
    return model.sign(seed, msg)


@functools.lru_cache(maxsize=None)
def model_verify(pk, msg, sig, strict):
    return model.verify(pk, msg, sig, strict)


def padded(msgs, stride):
    return [m + bytes(stride - len(m)) for m in msgs]


def as_limbs(engine, values):
    return engine.to_device(np.array([[(v >> (64 * j)) & (2**64 - 1) for j in range(4)] for v in values], dtype=np.uint64))


def from_limbs(t):
    from ecsimd_amd import Engine
    return [sum(int(w) << (64 * j) for j, w in enumerate(row)) for row in Engine.to_numpy(t)]


# ---- the field
def test_field_operations_against_integers_and_the_registered_modulus(engine):
    rng = random.Random(25519)
    pairs = [(a, b) for a in EDGE for b in EDGE] + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(2000)]
    a, b = [le32(x) for x, _ in pairs], [le32(y) for _, y in pairs]
    from ecsimd_amd.engine import register_modulus
    field = register_modulus(P, prime=True)
    ra, rb_ = as_limbs(engine, [x % P for x, _ in pairs]), as_limbs(engine, [y % P for _, y in pairs])      # the other path takes canonical residues
    second = dict(MUL=from_limbs(engine.mod_mul(field, ra, rb_)), ADD=from_limbs(engine.mod_add(field, ra, rb_)), SUB=from_limbs(engine.mod_sub(field, ra, rb_)),
                  SQR=from_limbs(engine.mod_mul(field, ra, ra)))
    for op, f in (("MUL", lambda x, y: x * y), ("ADD", lambda x, y: x + y), ("SUB", lambda x, y: x - y)):
        got = [int.from_bytes(o[0], "little") for o in raw(engine, op, a, b)]
        want = [f(x, y) % P for x, y in pairs]
        assert got == want, op
        assert got == second[op], op
    for op, f in (("SQR", lambda x: x * x), ("NEG", lambda x: -x), ("CANON", lambda x: x), ("INVERT", lambda x: pow(x, P - 2, P))):
        got = [int.from_bytes(o[0], "little") for o in raw(engine, op, a)]
        assert got == [f(x) % P for x, _ in pairs], op
        if op == "SQR":
            assert got == second[op]
    assert int.from_bytes(raw(engine, "INVERT", [le32(0), le32(P), le32(2 * P)])[1][0], "little") == 0          # the inverse of 0 is 0, whichever way 0 is written


def test_sqrt_ratio_on_every_class(engine):
    rng = random.Random(8032)
    us, vs, classes = [], [], []
    while len(us) < 600 or min(classes.count(c) for c in ("plain", "corrected", "none")) < 100:
        u, v = rng.getrandbits(256), rng.getrandbits(256)
        ok, x, corrected = model.sqrt_ratio(u, v)
        us.append(u); vs.append(v); classes.append("none" if not ok else "corrected" if corrected else "plain")
    for c in ("plain", "corrected", "none"):
        assert classes.count(c) >= 100, c                                                                      # the model puts 100 lanes in each class
    us += [0, 5, 0]; vs += [7, 0, 0]; classes += ["plain", "none", "plain"]                                  # u = 0: x = 0; v = 0: no root unless u = 0
    out = raw(engine, "SQRT_RATIO", [le32(u) for u in us], [le32(v) for v in vs])
    for u, v, c, o in zip(us, vs, classes, out):
        ok, x, _ = model.sqrt_ratio(u, v)
        assert o[1] == le32(int(ok)), (u, v)
        assert int.from_bytes(o[0], "little") == x, (u, v, c)
        if ok:
            assert (v * x * x - u) % P == 0


# ---- scalars
def test_reduction_of_512_bits_modulo_L(engine):
    rng = random.Random(252)
    top = (2**512 // L) * L
    values = [0, L - 1, L, L + 1, 2**252, 2**256 - 1, 2**512 - 1, top - 1, top + 1 if top + 1 < 2**512 else top - 2, 2**256, 2**256 * (L - 1)]
    values += [rng.getrandbits(512) for _ in range(500)]
    out = raw(engine, "SC_REDUCE", [le32(v & (2**256 - 1)) for v in values], [le32(v >> 256) for v in values])
    assert [int.from_bytes(o[0], "little") for o in out] == [v % L for v in values]


# ---- the group
def some_points(k):
    rng = random.Random(k)
    return [model.base_mult(rng.randrange(L)) for _ in range(k)]


def refused_encodings():
    out = [le32(P + i) for i in range(19)]                                  # y = p .. p + 18
    out += [le32(1 | (1 << 255)), le32((P - 1) | (1 << 255))]               # x = 0 with the sign bit set
    out += [le32(2), le32(2 | (1 << 255)), le32(7)]                         # no point with that y
    assert all(model.decode(e) is None for e in out)
    return out


def test_decode_and_encode(engine):
    keys = [c[2] for c in fixture()] + list(model.SMALL_ORDER) + some_points(20)
    bad = refused_encodings() + [le32((1 << 255) - 1), bytes([0xff]) * 32]
    out = raw(engine, "DECODE_ENCODE", keys + bad)
    for e, o in zip(keys, out):
        assert o == [e, le32(1)], e.hex()
    for e, o in zip(bad, out[len(keys):]):
        assert o == [ZERO32, le32(0)], e.hex()


def test_point_addition_and_doubling(engine):
    pts = some_points(24)
    ident, neg = le32(1), lambda e: model.encode(model.pt_neg(model.decode(e)))
    a = pts + pts[:8] + pts[:8] + pts[:8] + list(model.SMALL_ORDER) + [ident]
    b = pts[1:] + pts[:1] + pts[:8] + [neg(e) for e in pts[:8]] + [ident] * 8 + list(model.SMALL_ORDER) + [ident]       # P + Q, P + P, P + (-P), P + identity, torsion
    out = raw(engine, "POINT_ADD", a, b)
    for x, y, o in zip(a, b, out):
        assert o == [model.encode(model.pt_add(model.decode(x), model.decode(y))), le32(1)], (x.hex(), y.hex())
    assert all(o[0] == ident for o in out[32:40])                                                                        # P + (-P) is the identity
    out = raw(engine, "POINT_DBL", a)
    for x, o in zip(a, out):
        assert o == [model.encode(model.pt_dbl(model.decode(x))), le32(1)], x.hex()
    assert raw(engine, "POINT_ADD", [pts[0], le32(2)], [le32(2), pts[0]]) == [[ZERO32, le32(0)]] * 2


def test_fixed_base_multiplication(engine):
    rng = random.Random(99)
    ks = [0, 1, 2, 7, 8, L - 1, L, L + 1, 2**252, 2**254, 2**255 - 1, 2**256 - 1] + [rng.getrandbits(256) for _ in range(150)]
    ks += [int("8" * 64, 16), int("7" * 64, 16) % L, L - int("8" * 63, 16) % L]                                         # every digit at an end of its range
    out = raw(engine, "BASE_MULT", [le32(k) for k in ks])
    assert [o[0] for o in out] == [model.base_mult(k) for k in ks]
    assert out[0][0] == le32(1) and out[6][0] == le32(1) and out[1][0] == model.BY.to_bytes(32, "little")


def test_double_multiplication(engine):
    rng = random.Random(77)
    pts = some_points(40)
    base = model.encode(model.B)
    cases = [(0, 5, pts[0]), (5, 0, pts[1]), (0, 0, pts[2]), (3, L - 3, base), (L - 1, 1, base), (rng.randrange(L), 0, base)]
    cases += [(rng.getrandbits(256), rng.getrandbits(256), p) for p in pts]
    cases += [(rng.randrange(L), rng.randrange(L), e) for e in model.SMALL_ORDER]
    out = raw(engine, "DOUBLE_MULT", [le32(c[0]) for c in cases], [le32(c[1]) for c in cases], [c[2] for c in cases])
    for c, o in zip(cases, out):
        assert o == [model.double_mult(*c), le32(1)], c
    assert out[3][0] == le32(1) and out[4][0] == le32(1)                                                                 # s + h = L on B: the identity
    assert raw(engine, "DOUBLE_MULT", [le32(1)], [le32(1)], [le32(2)]) == [[ZERO32, le32(0)]]


# ---- points outside the prime-order subgroup: [k]B + T, T one of the seven non-zero torsion points
@functools.lru_cache(maxsize=None)
def mixed_points():
    """8 prime-order points times the 7 torsion points: (k, index of T, the point [k]B + T)"""
    rng = random.Random(56)
    tors = model.torsion()
    ks = [rng.randrange(1, L) for _ in range(8)]
    return tuple((k, j, model.mixed(model.base_point_mul(k), tors[j][1])) for k in ks for j in range(1, 8))


def from_parts(k, t):
    """the encoding of [k]B + t"""
    return model.encode(model.pt_add(model.base_point_mul(k), t))


def test_mixed_order_points_decode_add_and_double(engine):
    tors = model.torsion()
    mp = mixed_points()
    enc = [model.encode(m) for _, _, m in mp]
    assert len(set(enc)) == 56 and not set(enc) & set(model.SMALL_ORDER)
    assert raw(engine, "DECODE_ENCODE", enc) == [[e, le32(1)] for e in enc]
    rng = random.Random(57)
    a, b, want = [], [], []
    for i, (k, j, m) in enumerate(mp):
        k2 = rng.randrange(1, L)                                                                    # mixed + prime order
        a.append(enc[i]); b.append(model.base_mult(k2)); want.append(from_parts(k + k2, tors[j][1]))
        k3, j3, m3 = mp[(i + 9) % 56]                                                               # mixed + mixed: another k, another T
        a.append(enc[i]); b.append(enc[(i + 9) % 56]); want.append(from_parts(k + k3, model.pt_add(tors[j][1], tors[j3][1])))
        a.append(enc[i]); b.append(enc[i]); want.append(from_parts(2 * k, model.pt_dbl(tors[j][1])))  # mixed + itself, by the unified addition
        a.append(enc[i]); b.append(model.encode(model.pt_neg(m))); want.append(le32(1))             # mixed + its negative
        for e, t, _ in tors:                                                                        # mixed + torsion: -T among them, which leaves [k]B
            a.append(enc[i]); b.append(e); want.append(from_parts(k, model.pt_add(tors[j][1], t)))
            a.append(e); b.append(enc[i]); want.append(want[-1])
    out = raw(engine, "POINT_ADD", a, b)
    for x, y, w, o in zip(a, b, want, out):
        assert o == [w, le32(1)], (x.hex(), y.hex())
    assert want == [model.encode(model.pt_add(model.decode(x), model.decode(y))) for x, y in zip(a, b)]      # the parts and the points agree on the host
    assert all(want[20 * i:20 * i + 20].count(model.base_mult(k)) == 2 for i, (k, _, _) in enumerate(mp))    # adding -T, from either side, leaves [k]B
    out = raw(engine, "POINT_DBL", enc)
    for (k, j, m), o in zip(mp, out):
        assert o == [from_parts(2 * k, model.pt_dbl(tors[j][1])), le32(1)] and o[0] == model.encode(model.pt_dbl(m)), (k, j)


def test_double_multiplication_with_a_mixed_order_point(engine):
    """[s]B + [h mod L]([k]B + T) = [s + (h mod L) k]B + [(h mod L) mod 8]T: the expected value is made from the parts, the torsion part by the residue alone."""
    tors = model.torsion()
    rng = random.Random(58)
    cases = []
    for k, j, m in mixed_points():
        e = model.encode(m)
        sh = [(rng.randrange(L), (rng.randrange(L - 8) & ~7) + r) for r in range(8)]               # h congruent to each residue modulo 8
        sh += [(0, rng.randrange(1, L)), (rng.randrange(L), 8), (rng.randrange(L), L - 8)]         # s = 0; the table's last entry, [8]P, and its negative's residue
        sh += [(rng.randrange(L), int("7" * 40 + "8", 16)), (rng.randrange(L), int("7" * 62, 16))]  # 41 digits of -8; 62 digits of 7: both ends of the digit range
        sh += [(L + rng.randrange(L), L + rng.randrange(L)), (2**256 - 1, 2**256 - 1), (rng.randrange(15 * L, 2**256), rng.randrange(15 * L, 2**256)),
               (rng.randrange(L), L)]                                                              # scalars in [L, 2^256); h = L is h = 0
        cases += [(s, h, e, k, j) for s, h in sh]
    assert len(cases) == 56 * 17 and {c[1] % L % 8 for c in cases} == set(range(8))
    out = raw(engine, "DOUBLE_MULT", [le32(c[0]) for c in cases], [le32(c[1]) for c in cases], [c[2] for c in cases])
    for (s, h, e, k, j), o in zip(cases, out):
        hr = h % L
        assert o == [from_parts(s + hr * k, model.pt_mul(hr % 8, tors[j][1])), le32(1)], (s, h, e.hex())
    for c, o in list(zip(cases, out))[::41]:                                                        # ... and the model's plain double-and-add on the point itself
        assert o[0] == model.double_mult(c[0], c[1], c[2]), c[:3]


# ---- pubkey and sign
def sign_on_device(engine, seeds, msgs, stride=None, lens=False, want_pk=True, offset=0):
    """Signs msgs (a list of byte strings) with seeds; with lens the rows are `stride` wide and the lengths travel per lane; offset: the byte offset of the
    seed and message arrays inside their allocations."""
    import torch
    n = len(seeds)
    width = stride if stride is not None else (len(msgs[0]) if msgs else 0)
    sb = torch.zeros(32 * n + 8, dtype=torch.uint8, device=engine.tdev)
    st = sb[offset:offset + 32 * n].view(n, 32); st.copy_(dev_rows(engine, seeds, 32))
    mb = torch.zeros(max(width, 1) * n + 8, dtype=torch.uint8, device=engine.tdev)
    mt = mb[offset:offset + width * n].view(n, width)
    if width:
        mt.copy_(dev_rows(engine, padded(msgs, width), width))
    lt = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=engine.tdev) if lens else None
    sig, pk = engine.ed25519_sign(st, mt, lens=lt, want_pk=want_pk)
    return host_rows(sig), (host_rows(pk) if want_pk else None), (st, mt, lt)


def test_the_fixture_bit_for_bit_equal_lengths_and_per_lane_lengths(engine):
    import torch
    fx = fixture()
    by_len = {}
    for c in fx:
        by_len.setdefault(len(c[1]), []).append(c)
    assert set(LENGTHS) <= set(by_len) and 2 in by_len
    for length, cases in sorted(by_len.items()):                                                    # equal lengths: one call per length
        sig, pk, _ = sign_on_device(engine, [c[0] for c in cases], [c[1] for c in cases])
        assert sig == [c[3] for c in cases] and pk == [c[2] for c in cases], length
        assert host_rows(engine.ed25519_pubkey(dev_rows(engine, [c[0] for c in cases], 32))) == [c[2] for c in cases]
    # ... and all of them in one batch through lens, once aligned and once at an odd base with an odd stride
    for stride, offset in ((304, 0), (301, 1)):
        sig, pk, (st, mt, lt) = sign_on_device(engine, [c[0] for c in fx], [c[1] for c in fx], stride=stride, lens=True, offset=offset)
        assert sig == [c[3] for c in fx] and pk == [c[2] for c in fx], (stride, offset)
        sig2, none, _ = sign_on_device(engine, [c[0] for c in fx], [c[1] for c in fx], stride=stride, lens=True, want_pk=False, offset=offset)
        assert sig2 == sig and none is None
        gt, kt = dev_rows(engine, sig, 64), dev_rows(engine, pk, 32)
        assert engine.ed25519_verify(kt, mt, gt, lens=lt).cpu().tolist() == [1] * len(fx)
        # unaligned keys and signatures as well
        gb = torch.zeros(64 * len(fx) + 8, dtype=torch.uint8, device=engine.tdev); g1 = gb[3:3 + 64 * len(fx)].view(-1, 64); g1.copy_(gt)
        kb = torch.zeros(32 * len(fx) + 8, dtype=torch.uint8, device=engine.tdev); k1 = kb[1:1 + 32 * len(fx)].view(-1, 32); k1.copy_(kt)
        assert engine.ed25519_verify(k1, mt, g1, lens=lt).cpu().tolist() == [1] * len(fx)
        assert host_rows(engine.ed25519_pubkey(st)) == [c[2] for c in fx]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_batch_sizes(engine, n):
    rng = random.Random(64)
    seeds = [rng.randbytes(32) for _ in range(64)]
    msgs = [rng.randbytes(LENGTHS[j % len(LENGTHS)]) for j in range(64)]
    s, m = [seeds[i % 64] for i in range(n)], [msgs[i % 64] for i in range(n)]
    sig, pk, (st, mt, lt) = sign_on_device(engine, s, m, stride=300, lens=True)
    want = [model_sign(a, b) for a, b in zip(s, m)]
    assert sig == [w[0] for w in want] and pk == [w[1] for w in want]
    assert host_rows(engine.ed25519_pubkey(st)) == pk
    assert engine.ed25519_verify(dev_rows(engine, pk, 32), mt, dev_rows(engine, sig, 64), lens=lt).cpu().tolist() == [1] * n


@functools.lru_cache(maxsize=None)
def every_length():
    """(seeds, messages, the model's (signature, public key)) for the lengths 0 .. 272, one lane each, 16 seeds in turn: both heads' block boundaries (the
    32-byte head's at 79 / 80, 207 / 208, the 64-byte head's at 47 / 48, 175 / 176), the word boundaries between them, and one block more."""
    rng = random.Random(272)
    pool = [rng.randbytes(32) for _ in range(16)]
    seeds = tuple(pool[i % 16] for i in range(273))
    msgs = tuple(rng.randbytes(i) for i in range(273))
    return seeds, msgs, tuple(model_sign(s, m) for s, m in zip(seeds, msgs))


@pytest.mark.parametrize("stride,offset", [(272, 0), (273, 1)])
def test_every_message_length_up_to_272_in_one_batch(engine, stride, offset):
    import torch
    seeds, msgs, want = every_length()
    sig, pk, (st, mt, lt) = sign_on_device(engine, list(seeds), list(msgs), stride=stride, lens=True, offset=offset)
    assert mt.data_ptr() % 4 == offset and lt.cpu().tolist() == list(range(273))
    wrong = [i for i in range(273) if (sig[i], pk[i]) != want[i]]
    assert not wrong, wrong
    gt, kt = at_offset(engine, sig, 64, offset), at_offset(engine, pk, 32, offset)
    assert engine.ed25519_verify(kt, mt, gt, lens=lt).cpu().tolist() == [1] * 273
    # one byte fewer is another message: every lane but the empty one is refused (the length is read per lane, exactly)
    assert engine.ed25519_verify(kt, mt, gt, lens=torch.clamp(lt - 1, min=0)).cpu().tolist() == [1] + [0] * 272


# ---- verify
def verify_lanes():
    """(kind, pk, msg, sig) for about 1 000 lanes."""
    rng = random.Random(1000)
    fx = fixture()
    lanes = []
    flip = lambda b, bit: (int.from_bytes(b, "little") ^ (1 << bit)).to_bytes(len(b), "little")
    for rep in range(13):
        for seed, msg, pk, sig in fx:
            lanes.append(("valid", pk, msg, sig))
    for j, (seed, msg, pk, sig) in enumerate(fx):
        s = int.from_bytes(sig[32:], "little")
        lanes.append(("flip pk", flip(pk, rng.randrange(256)), msg, sig))
        lanes.append(("flip R", pk, msg, flip(sig[:32], rng.randrange(256)) + sig[32:]))
        lanes.append(("flip s", pk, msg, sig[:32] + flip(sig[32:], rng.randrange(252))))
        if msg:
            lanes.append(("flip message", pk, flip(msg, rng.randrange(8 * len(msg))), sig))
            lanes.append(("message shorter", pk, msg[:-1], sig))
        lanes.append(("message longer", pk, msg + b"\x00", sig))
        if s + L < 2**256:
            lanes.append(("s + L", pk, msg, sig[:32] + le32(s + L)))
        lanes.append(("s = L", pk, msg, sig[:32] + le32(L)))
    seed, msg, pk, sig = fx[5]
    for e in refused_encodings():
        lanes.append(("A refused", e, msg, sig))
    lanes.append(("R non-canonical", model.SMALL_ORDER[0], b"m", le32(P + 1) + le32(0)))              # 1 written as p + 1 under A = identity, s = 0: the equation holds for the point
    for a in model.SMALL_ORDER:                                                                       # s = 0: R = -k A, another small-order point -- found by trying messages
        for r in model.SMALL_ORDER:
            for t in range(4):
                lanes.append(("small order", a, bytes([t]), r + le32(0)))
    for a in model.SMALL_ORDER[:4]:
        lanes.append(("small-order A, honest R", a, msg, sig))
    for r in model.SMALL_ORDER:
        lanes.append(("small-order R, honest A", pk, msg, r + sig[32:]))
    return lanes


def test_one_batch_of_every_kind_in_both_flag_settings(engine):
    lanes = verify_lanes()
    assert 900 <= len(lanes) <= 1200
    stride = 304
    pk = dev_rows(engine, [l[1] for l in lanes], 32); sig = dev_rows(engine, [l[3] for l in lanes], 64)
    import torch
    msgs = dev_rows(engine, padded([l[2] for l in lanes], stride), stride)
    lens = torch.tensor([len(l[2]) for l in lanes], dtype=torch.int32, device=engine.tdev)
    for strict in (False, True):
        got = engine.ed25519_verify(pk, msgs, sig, lens=lens, reject_small_order=strict).cpu().tolist()
        want = [int(model_verify(l[1], l[2], l[3], strict)) for l in lanes]
        wrong = [(i, lanes[i][0]) for i in range(len(lanes)) if got[i] != want[i]]
        assert not wrong, (strict, wrong[:10])
        assert 0 in want and 1 in want
        kinds = {l[0] for l in lanes}
        assert len(kinds) >= 13
        by_kind = {k: {w for l, w in zip(lanes, want) if l[0] == k} for k in kinds}
        assert by_kind["valid"] == {1}
        for k in kinds - {"valid", "small order"}:
            assert by_kind[k] == {0}, k
        assert by_kind["small order"] == ({0} if strict else {0, 1})                                  # the default rule set accepts the ones whose equation holds
    assert model.verify(model.SMALL_ORDER[0], b"anything", model.SMALL_ORDER[0] + le32(0)) and not model.verify(model.SMALL_ORDER[0], b"anything", model.SMALL_ORDER[0] + le32(0), True)


# ---- the verdict fixture: what libcrypto and the model said of every lane when it was minted; no model runs here
@functools.lru_cache(maxsize=None)
def verdicts():
    return tuple(json.load(open(model.VERDICTS_PATH))["records"])


@pytest.mark.parametrize("stride,offset", [(16, 0), (17, 1)])
def test_the_verdict_fixture_in_one_batch_in_both_flag_settings(engine, stride, offset):
    """offset 1, stride 17: the keys, the signatures, the messages and the verdicts all start at an odd address (the lengths stay word aligned, as the
    header asks), and the messages' rows fall on every residue modulo 4."""
    import torch
    recs = verdicts()
    n = len(recs)
    assert 1000 <= n <= 1500
    msgs = [bytes.fromhex(r["message"]) for r in recs]
    assert max(len(m) for m in msgs) == 16 and min(len(m) for m in msgs) == 0
    pk = at_offset(engine, [bytes.fromhex(r["public_key"]) for r in recs], 32, offset)
    sig = at_offset(engine, [bytes.fromhex(r["signature"]) for r in recs], 64, offset)
    mt = at_offset(engine, padded(msgs, stride), stride, offset)
    lens = torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=engine.tdev)
    for flags, column in ((0, "model"), (1, "model_strict")):
        buf = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device=engine.tdev)
        ok = buf[offset:offset + n]
        engine._bind_stream()
        engine._check(engine.lib.ecsimd_ed25519_verify(engine.ctx, C.c_void_p(pk.data_ptr()), C.c_void_p(mt.data_ptr()), C.c_size_t(stride), C.c_size_t(stride),
                                                      C.c_void_p(lens.data_ptr()), C.c_void_p(sig.data_ptr()), C.c_void_p(ok.data_ptr()), C.c_size_t(n), C.c_int(flags)),
                      "ed25519_verify")
        got = ok.cpu().tolist()
        wrong = [(i, recs[i]["kind"], recs[i].get("orders"), got[i]) for i in range(n) if got[i] != recs[i][column]]
        assert not wrong, (column, len(wrong), wrong[:10])
        assert set(buf[:offset].cpu().tolist()) <= {0xA5} and set(buf[offset + n:].cpu().tolist()) == {0xA5}      # nothing outside the n verdicts was written
        if flags == 0:
            assert all(g == r["libcrypto"] for g, r in zip(got, recs) if not r.get("divergent"))                  # libcrypto's verdict, where the header claims it
            assert [r["kind"] for g, r in zip(got, recs) if g != r["libcrypto"]] == [model.DIVERGENT_KIND] * 2
        for kind in model.MIXED_KINDS[::2] + ("small order",) * (1 - flags):
            assert {g for g, r in zip(got, recs) if r["kind"] == kind} == {0, 1}, kind                            # both verdicts came out of the device


def test_one_launch_sequence_across_the_chunk_boundary(engine):
    """verify goes through the workspace in chunks of 2^20 lanes: 64 distinct signatures tiled over 2^20 + 70 lanes, bad lanes on both sides of the boundary."""
    import torch
    chunk, n = 1 << 20, (1 << 20) + 70
    fx = fixture()
    rng = random.Random(20)
    base = [(rng.randbytes(32), rng.randbytes(40)) for _ in range(64 - len(fx))]
    # every tile record: a 40-byte row, the lane's length in lens
    rows = [(model_sign(s, m)[1], m, 40, model_sign(s, m)[0]) for s, m in base] + [(c[2], c[1][:40].ljust(40, b"\0"), min(len(c[1]), 40), model_sign(c[0], c[1][:40])[0]) for c in fx]
    assert len(rows) == 64
    reps = (n + 63) // 64
    pk = dev_rows(engine, [r[0] for r in rows], 32).repeat(reps, 1)[:n].contiguous()
    msgs = dev_rows(engine, [r[1] for r in rows], 40).repeat(reps, 1)[:n].contiguous()
    sig = dev_rows(engine, [r[3] for r in rows], 64).repeat(reps, 1)[:n].contiguous()
    lens = torch.tensor([r[2] for r in rows], dtype=torch.int32, device=engine.tdev).repeat(reps)[:n].contiguous()
    bad = [0, 5, chunk - 64, chunk - 1, chunk, chunk + 1, chunk + 63, n - 1]
    for b in bad:
        sig[b, 7] ^= 1
    got = engine.ed25519_verify(pk, msgs, sig, lens=lens)
    want = torch.ones(n, dtype=torch.uint8, device=engine.tdev)
    want[torch.tensor(bad, device=engine.tdev)] = 0
    assert torch.equal(got, want), (got != want).nonzero()[:10].tolist()


# ---- graph capture
def test_replay_of_the_three_calls_and_the_refusal_before_any_warm_up():
    import torch
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    n, stride = 130, 96
    rng = random.Random(3)
    sets = []
    for i in range(3):
        seeds = [rng.randbytes(32) for _ in range(n)]
        msgs = [rng.randbytes(rng.choice((0, 1, 47, 48, 64, 95, 96))) for _ in range(n)]
        want = [model_sign(s, m) for s, m in zip(seeds, msgs)]
        sigs = [w[0] for w in want]
        bad = {7 + i, 64, 129 - i}
        sigs = [bytes([sg[0] ^ 1]) + sg[1:] if j in bad else sg for j, sg in enumerate(sigs)]
        sets.append(dict(seeds=seeds, msgs=msgs, want=want, sigs=sigs, ok=[int(j not in bad) for j in range(n)]))
    eng = Engine(0)
    try:
        def load(i, b=None):
            s = sets[i]
            t = dict(seeds=dev_rows(eng, s["seeds"], 32), msgs=dev_rows(eng, padded(s["msgs"], stride), stride), sigs=dev_rows(eng, s["sigs"], 64),
                     pks=dev_rows(eng, [w[1] for w in s["want"]], 32), lens=torch.tensor([len(m) for m in s["msgs"]], dtype=torch.int32, device=eng.tdev))
            if b is None:
                return t
            for k in t:
                b[k].copy_(t[k])
            return b

        def run(b):
            sig, pk = eng.ed25519_sign(b["seeds"], b["msgs"], lens=b["lens"])
            return dict(sig=sig, pk=pk, pk2=eng.ed25519_pubkey(b["seeds"]), ok=eng.ed25519_verify(b["pks"], b["msgs"], b["sigs"], lens=b["lens"]))

        bufs = load(0)
        # before any warm-up: each call refuses under capture, names it, and leaves the capture valid
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        said = {}
        with torch.cuda.stream(side):
            with torch.cuda.graph(g0, stream=side):
                for name, call in (("pubkey", lambda: eng.ed25519_pubkey(bufs["seeds"])), ("sign", lambda: eng.ed25519_sign(bufs["seeds"], bufs["msgs"], lens=bufs["lens"])),
                                   ("verify", lambda: eng.ed25519_verify(bufs["pks"], bufs["msgs"], bufs["sigs"], lens=bufs["lens"]))):
                    try:
                        call(); said[name] = "it did not refuse"
                    except EcsimdHipError as e:
                        said[name] = str(e)
                marker = bufs["lens"] + 1                                        # the capture is still valid: this node is recorded
        torch.cuda.synchronize()
        for name, text in said.items():
            assert "(-1)" in text and "capture" in text, (name, text)            # ECSIMD_HIP_ERR_BAD_ARG
        g0.replay(); torch.cuda.synchronize()
        assert torch.equal(marker, bufs["lens"] + 1)
        del g0
        run(bufs); torch.cuda.synchronize()                                      # the warm-up at the capture's batch size
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out = run(bufs)
        torch.cuda.synchronize()
        for i in (1, 2):
            load(i, bufs); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            s = sets[i]
            assert host_rows(out["sig"]) == [w[0] for w in s["want"]], i
            assert host_rows(out["pk"]) == [w[1] for w in s["want"]] == host_rows(out["pk2"]), i
            assert out["ok"].cpu().tolist() == s["ok"], i
        del g
    finally:
        eng.close()


# ---- the workspace after the secret calls
@pytest.mark.parametrize("call", ["sign", "pubkey"])
def test_the_used_prefix_of_the_workspace_is_zero_afterwards(call):
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    try:
        n = 300
        rng = random.Random(11)
        seeds = dev_rows(eng, [rng.randbytes(32) for _ in range(n)], 32)
        msgs = dev_rows(eng, [rng.randbytes(33) for _ in range(n)], 33)
        run = (lambda: eng.ed25519_sign(seeds, msgs)) if call == "sign" else (lambda: eng.ed25519_pubkey(seeds))
        run(); torch.cuda.synchronize()
        ptr, size = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        used = n * (128 if call == "sign" else 32)                               # a, r and both encodings / a alone: 32 bytes each per lane
        assert ptr.value and size.value >= used
        fill = np.full(size.value, 0xA5, dtype=np.uint8)
        eng._bind_stream()
        eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(size.value)), "memcpy_h2d")
        run(); torch.cuda.synchronize()
        back = np.empty(size.value, dtype=np.uint8)
        eng._check(eng.lib.ecsimd_hip_memcpy_d2h(eng.ctx, back.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(size.value)), "memcpy_d2h")
        assert not back[:used].any(), np.flatnonzero(back[:used])[:8]
        assert (back[used:] == 0xA5).all()                                       # ... and nothing behind it was touched
    finally:
        eng.close()


def test_empty_batches_and_refused_arguments(engine):
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    e8 = lambda w: torch.zeros((0, w), dtype=torch.uint8, device=engine.tdev)
    assert engine.ed25519_pubkey(e8(32)).shape == (0, 32)
    sig, pk = engine.ed25519_sign(e8(32), e8(5))
    assert sig.shape == (0, 64) and pk.shape == (0, 32)
    assert engine.ed25519_verify(e8(32), e8(5), e8(64)).shape == (0,)
    one = torch.zeros((1, 32), dtype=torch.uint8, device=engine.tdev)
    with pytest.raises(EcsimdHipError, match="unknown flag"):
        engine._check(engine.lib.ecsimd_ed25519_verify(engine.ctx, C.c_void_p(one.data_ptr()), None, C.c_size_t(0), C.c_size_t(0), None, C.c_void_p(one.data_ptr()),
                                                      C.c_void_p(one.data_ptr()), C.c_size_t(1), C.c_int(2)), "ed25519_verify")
    engine.set_ref_square_compat(True)                                           # accepted: the same bytes
    try:
        c = fixture()[0]
        assert host_rows(engine.ed25519_pubkey(dev_rows(engine, [c[0]], 32))) == [c[2]]
    finally:
        engine.set_ref_square_compat(False)
