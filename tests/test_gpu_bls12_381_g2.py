"""GPU suite for BLS12-381 G2 (include/ecsimd_bls12_381_g2.h).  Every expected value comes from tools/bls12_381_g2_model.py (Python integers, Fp2 as pairs, the
affine textbook law) or from tests/golden/bls12_381_g2_vectors.json, which that model writes; never from the library.  Layer by layer through ecsimd_bls381_g2_raw
-- the extension field against Python integers on the representation's bounds in both components, inversion and square roots of every class, the group law on
every exceptional pair --, then the encodings with every kind of malformed record, the subgroup test against [r] Q = infinity, the scalar product with integer
semantics, the sum on all routes (the same bytes from each) with the batches that cut runs, fire the doubling branch inside the buckets and sum buckets to
infinity, the point sum from both encodings, call hygiene, and graph capture.

MSM terms are Q_i = (a0 + i d) G2, built with one affine addition per term, so an expected sum is ONE scalar product: (sum k_i (a0 + i d) mod r) G2."""
import functools
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_381_g2_model as model   # noqa: E402
from bls12_381_model import fe_sqrt   # noqa: E402

pytestmark = pytest.mark.gpu
P, R, G, INF = model.P, model.R, model.G, model.INF
OP = dict(FE2_MUL=0, FE2_SQR=1, FE2_ADD=2, FE2_SUB=3, FE2_NEG=4, FE2_INVERT=5, FE2_SQRT=6, FE2_CANON=7, POINT_ADD=8, POINT_DBL=9, POINT_MADD=10)
ALL = 2**384 - 1
AUTO, BUCKETS, LANES = 0, 1, 2
i2b = lambda v: v.to_bytes(48, "big")
b2i = lambda b: int.from_bytes(b, "big")
NMAX = 4097
A0, D = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcdef % R, 0x0fedcba987654321fedcba987654321fedcba987654321fedcba987654321 % R
red = lambda a: (a[0] % P, a[1] % P)


@functools.lru_cache(maxsize=None)
def fixture():
    return json.load(open(model.FIXTURE))


@functools.lru_cache(maxsize=None)
def world():
    """The NMAX terms and their 256-bit scalars, once."""
    rng = random.Random(12381)
    pts, acc, step = [], model.mul(A0, G), model.mul(D, G)
    for _ in range(NMAX):
        pts.append(acc); acc = model.add(acc, step)
    return dict(pts=pts, enc=[model.encode192(p) for p in pts], k=[rng.getrandbits(256) for _ in range(NMAX)])


def expected_sum(ks, bits=256, idx=None):
    idx = range(len(ks)) if idx is None else idx
    return model.mul(sum((k % (1 << bits)) * (A0 + i * D) for k, i in zip(ks, idx)) % R, G)


@pytest.fixture(scope="module")
def eng():
    from ecsimd_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def dev_rows(engine, rows, width):
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    return torch.from_numpy(a).to(engine.tdev)


def empty_rows(engine, width):
    return dev_rows(engine, [bytes(width)], width)[:0]


def at_offset(engine, rows, width, offset=1):
    import torch
    n = len(rows)
    buf = torch.zeros(width * n + 8, dtype=torch.uint8, device=engine.tdev)
    view = buf[offset:offset + width * n].view(n, width)
    view.copy_(dev_rows(engine, rows, width))
    assert view.data_ptr() % 4 == offset % 4
    return view


def host_rows(t):
    return [bytes(r) for r in t.cpu().numpy()]


def dev_scalars(engine, ks):
    a = np.array([[(k >> (64 * j)) & 0xffffffffffffffff for j in range(4)] for k in ks], dtype=np.uint64).reshape(len(ks), 4)
    return engine.to_device(a)


def raw(engine, op, rows):
    """rows: one list of 384-bit integers per lane (an Fp2 operand is two of them, c0 then c1); returns the output records as integers per lane."""
    rec = [b"".join(i2b(v) for v in row) for row in rows]
    out = host_rows(engine.bls12_381_g2_raw(OP[op], dev_rows(engine, rec, 48 * len(rows[0]))))
    return [[b2i(o[k:k + 48]) for k in range(0, len(o), 48)] for o in out]


def pt5(pt):
    return [0, 0, 0, 0, 1] if pt is INF else [pt[0][0], pt[0][1], pt[1][0], pt[1][1], 0]


def msm(engine, ks, encs, bits=255, alg=BUCKETS):
    out, finite, invalid = engine.bls12_381_g2_msm(dev_scalars(engine, ks), dev_rows(engine, encs, 192) if encs else empty_rows(engine, 192), bits=bits, alg=alg, want_invalid=True)
    return bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())


def sum_result(pt, invalid=0):
    return (model.encode192(pt), 0 if pt is INF else 1, invalid)


def dec(r):
    return model.decode192(bytes.fromhex(r["uncompressed"]))


# ---- the field, through raw
def test_the_field_equals_python_integers_on_random_operands_and_the_bounds(eng):
    rng = random.Random(1)
    bounds = [int(v, 16) for v in fixture()["field_operands"]]
    key = [0, 1, P - 1, P, ALL]
    for want in key:
        assert want in bounds
    rnd2 = lambda: (rng.getrandbits(384), rng.getrandbits(384))
    elems = [(x, y) for x in key for y in key]                                                      # the bounds in both components
    pairs = [(rnd2(), rnd2()) for _ in range(2000)] + [(a, b) for a in elems for b in elems] + [((x, y), (y, x)) for x in bounds for y in bounds]
    rows = [list(a + b) for a, b in pairs]
    assert raw(eng, "FE2_MUL", rows) == [list(model.f2_mul(a, b)) for a, b in pairs]
    assert raw(eng, "FE2_ADD", rows) == [list(model.f2_add(a, b)) for a, b in pairs]
    assert raw(eng, "FE2_SUB", rows) == [list(model.f2_sub(a, b)) for a, b in pairs]
    one = [a for a, _ in pairs[:2000]] + elems + [(x, y) for x in bounds for y in bounds]
    rows = [list(a) for a in one]
    assert raw(eng, "FE2_SQR", rows) == [list(model.f2_sqr(a)) for a in one]
    assert raw(eng, "FE2_NEG", rows) == [list(model.f2_neg(a)) for a in one]
    assert raw(eng, "FE2_CANON", rows) == [list(red(a)) for a in one]


def test_inversion_and_square_roots(eng):
    rng = random.Random(2)
    rnd2 = lambda: (rng.getrandbits(384), rng.getrandbits(384))
    key = [0, 1, P - 1, P, ALL]
    a = [(x, y) for x in key for y in key] + [rnd2() for _ in range(39)]
    got = raw(eng, "FE2_INVERT", [list(v) for v in a])
    assert got == [list(model.f2_inv(v)) for v in a]                                                # (0, 0), (p, p), (0, p), (p, 0) -> 0
    assert all(red(v) == (0, 0) or model.f2_mul(v, tuple(g)) == (1, 0) for v, g in zip(a, got))
    qr = [v for v in range(2, 60) if fe_sqrt(v) is not None][:6]
    nqr = [v for v in range(2, 60) if fe_sqrt(v) is None][:6]
    in_fp = [(0, 0), (P, P), (1, 0), (P - 1, 0), (4, 0), (P + 4, P)] + [(v, 0) for v in qr + nqr] + [(rng.randrange(P), 0) for _ in range(10)]
    squares = [model.f2_sqr(rnd2()) for _ in range(24)] + [(0, 1), (0, 2), (0, P - 1)]
    others = [red(rnd2()) for _ in range(48)]
    vals = in_fp + squares + others
    got = raw(eng, "FE2_SQRT", [list(v) for v in vals])
    flags = []
    for v, (c0, c1, flag) in zip(vals, got):
        have = model.f2_sqrt(v) is not None
        assert flag == (1 if have else 0), v
        assert not have or model.f2_sqr((c0, c1)) == red(v), v                                      # a root whenever one exists
        flags.append(flag)
    assert all(flags[:len(in_fp) + len(squares)])                                                   # every element of Fp and every square has a root
    assert 0 < sum(flags[len(in_fp) + len(squares):]) < len(others)                                 # squares and non-squares among the random ones
    for v, (c0, c1, flag) in zip(vals, got):
        if v[1] % P == 0 and v[0] % P in qr:
            assert c1 == 0 and c0 * c0 % P == v[0] % P                                              # a residue of Fp: the real root
        if v[1] % P == 0 and v[0] % P in nqr:
            assert c0 == 0 and -c1 * c1 % P == v[0] % P                                             # a non-residue of Fp: the purely imaginary root u sqrt(-a)


# ---- the group law, through raw
def test_the_group_law_on_every_kind_of_pair(eng):
    w = world()["pts"]
    fx = fixture()
    off, tors = dec(fx["off_subgroup"][0]), dec(fx["h_torsion"])
    pts = [INF, G, model.neg(G), w[0], w[1], model.neg(w[1]), model.add(G, G), off, model.neg(off), tors, dec(fx["real_y"]), dec(fx["imaginary_y"])]
    pairs = [(a, b) for a in pts for b in pts]                                                    # generic, P + P, P + (-P), inf + P, P + inf, inf + inf
    assert raw(eng, "POINT_ADD", [pt5(a) + pt5(b) for a, b in pairs]) == [pt5(model.add(a, b)) for a, b in pairs]
    assert raw(eng, "POINT_DBL", [pt5(a) for a in pts]) == [pt5(model.add(a, a)) for a in pts]
    mixed = [(a, b) for a in pts for b in pts if b is not INF]                                    # the accumulator equal to the term and to its negative among them
    assert raw(eng, "POINT_MADD", [pt5(a) + pt5(b)[:4] for a, b in mixed]) == [pt5(model.add(a, b)) for a, b in mixed]
    assert any(a == b for a, b in mixed) and any(a is not INF and a == model.neg(b) for a, b in mixed)


# ---- the encodings
def test_the_fixture_round_trips_bit_for_bit_and_malformed_records_are_refused(eng):
    fx = fixture()
    recs = model.point_records(fx)
    u, c = [bytes.fromhex(r["uncompressed"]) for r in recs], [bytes.fromhex(r["compressed"]) for r in recs]
    assert u[0][0] == 0x40 and c[0][0] == 0xc0 and {x[0] & 0x20 for x in c[1:]} == {0, 0x20}       # infinity in both forms, both values of the sort bit
    bad_u, bad_c = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"]], [bytes.fromhex(m["bytes"]) for m in fx["malformed_compressed"]]
    out, ok = eng.bls12_381_g2_decompress(dev_rows(eng, c + bad_c, 96))
    assert host_rows(out) == u + [bytes(192)] * len(bad_c) and ok.cpu().tolist() == [1] * len(c) + [0] * len(bad_c)
    out, ok = eng.bls12_381_g2_compress(dev_rows(eng, u + bad_u, 192))
    assert host_rows(out) == c + [bytes(96)] * len(bad_u) and ok.cpu().tolist() == [1] * len(u) + [0] * len(bad_u)
    w = world()
    out, ok = eng.bls12_381_g2_compress(dev_rows(eng, w["enc"][:300], 192))                       # more than one block
    assert host_rows(out) == [model.encode96(p) for p in w["pts"][:300]] and ok.cpu().tolist() == [1] * 300
    back, ok = eng.bls12_381_g2_decompress(out)
    assert host_rows(back) == w["enc"][:300] and ok.cpu().tolist() == [1] * 300


def test_g2_check_is_the_definition(eng):
    fx = fixture()
    recs = model.point_records(fx)
    bad = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"]]
    on, sub = eng.bls12_381_g2_check(dev_rows(eng, [bytes.fromhex(r["uncompressed"]) for r in recs] + bad, 192))
    want = [model.in_subgroup(dec(r)) for r in recs]
    assert want == [r["in_subgroup"] for r in recs] and want.count(False) >= 5 and want[0] is True   # infinity is in the subgroup
    assert on.cpu().tolist() == [1] * len(recs) + [0] * len(bad) and sub.cpu().tolist() == [int(x) for x in want] + [0] * len(bad)


def test_g2_mul_has_integer_semantics(eng):
    rng = random.Random(3)
    w = world()
    off = dec(fixture()["off_subgroup"][1])
    ks = [0, 1, 2, R - 1, R, R + 1, 2**256 - 1] + [rng.getrandbits(256) for _ in range(64)]
    pts = [w["pts"][i] for i in range(len(ks))] + [off] * 8 + [INF]
    ks = ks + [0, 1, 2, R - 1, R, R + 1, 2**256 - 1, rng.getrandbits(256), 5]
    encs = [model.encode192(p) for p in pts] + [bytes.fromhex(fixture()["malformed_uncompressed"][0]["bytes"])]
    out, ok = eng.bls12_381_g2_mul(dev_scalars(eng, ks + [7]), dev_rows(eng, encs, 192))
    assert host_rows(out) == [model.encode192(model.mul(k, p)) for k, p in zip(ks, pts)] + [bytes(192)] and ok.cpu().tolist() == [1] * len(ks) + [0]
    assert model.mul(R, off) is not INF
    kb = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks[:9]), dtype=np.uint8).reshape(9, 32).copy()   # Engine converts from bytes
    import torch
    out2, _ = eng.bls12_381_g2_mul(torch.from_numpy(kb).to(eng.tdev), dev_rows(eng, encs[:9], 192))
    assert host_rows(out2) == host_rows(out)[:9]


# ---- the sum
@pytest.mark.parametrize("n", [0, 1, 2, 3, 16, 17, 33, 257, 1000, 4097])
def test_g2_msm_every_route_gives_the_models_bytes(eng, n):
    w = world()
    ks = w["k"][:n]
    want = sum_result(expected_sum(ks, 255))
    assert msm(eng, ks, w["enc"][:n], 255, BUCKETS) == want
    assert msm(eng, ks, w["enc"][:n], 255, LANES) == want
    plan = eng.bls12_381_g2_msm_plan(n, 255, AUTO)
    assert plan["route"] in (BUCKETS, LANES) and msm(eng, ks, w["enc"][:n], 255, AUTO) == want    # AUTO is the route the plan names: the same bytes either way
    if n == 1000:
        assert eng.bls12_381_g2_msm_plan(n, 255, BUCKETS)["L"] == 8                                # runs are cut: combine runs


@pytest.mark.parametrize("bits", [1, 7, 128, 256])
def test_g2_msm_reads_only_the_low_bits(eng, bits):
    w = world()
    ks = [k | (1 << 255) | (0xdead << 200) for k in w["k"][:257]]                                 # garbage in the high bits
    want = sum_result(expected_sum(ks, bits))
    assert msm(eng, ks, w["enc"][:257], bits, BUCKETS) == want and msm(eng, ks, w["enc"][:257], bits, LANES) == want


@functools.lru_cache(maxsize=None)
def special_batches():
    w = world()
    n = 1000
    rng = random.Random(4)
    k0 = rng.getrandbits(255)
    out = {}
    out["every scalar equal"] = ([k0] * n, w["enc"][:n], sum_result(expected_sum([k0] * n, 255)))
    out["every point equal"] = (w["k"][:n], [w["enc"][5]] * n, sum_result(model.mul(sum(k % 2**255 for k in w["k"][:n]) * (A0 + 5 * D) % R, G)))
    neg5 = model.encode192(model.neg(w["pts"][5]))
    out["alternating Q and -Q"] = ([k0] * n, [w["enc"][5] if i % 2 == 0 else neg5 for i in range(n)], sum_result(INF))
    out["all scalars zero"] = ([0] * n, w["enc"][:n], sum_result(INF))
    ks = list(w["k"][:n - 1]); tot = sum((k % 2**255) * (A0 + i * D) for i, k in enumerate(ks)) % R
    last = (-tot * pow(A0 + (n - 1) * D, -1, R)) % R
    assert last < 2**255
    out["a total of infinity"] = (ks + [last], w["enc"][:n], sum_result(INF))
    fx = fixture()
    bad = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"][:7]]
    offs = [dec(r) for r in fx["off_subgroup"][:2]]
    encs, ks = list(w["enc"][:n]), list(w["k"][:n])
    where_bad = [0, 10, 107, 204, 301, 398, n - 1]                                                  # both ends and the middle
    for j, b in zip(where_bad, bad):
        encs[j] = b
    where_inf = [20 + 101 * j for j in range(5)]
    for j in where_inf:
        encs[j] = model.encode192(INF)
    where_off = (333, 777)
    for j, o in zip(where_off, offs):
        encs[j] = model.encode192(o)
    skipped = set(where_bad) | set(where_inf) | set(where_off)
    assert len(skipped) == 14
    idx = [i for i in range(n) if i not in skipped]
    acc = expected_sum([ks[i] for i in idx], 255, idx)
    for j, o in zip(where_off, offs):
        acc = model.add(acc, model.mul(ks[j] % 2**255, o))                                       # the sum is over the integers
    out["malformed, infinite and off-subgroup terms"] = (ks, encs, sum_result(acc, 7))
    return out


@pytest.mark.parametrize("name", ["every scalar equal", "every point equal", "alternating Q and -Q", "all scalars zero", "a total of infinity",
                                  "malformed, infinite and off-subgroup terms"])
def test_g2_msm_special_batches(eng, name):
    ks, encs, want = special_batches()[name]
    assert eng.bls12_381_g2_msm_plan(1000, 255, BUCKETS)["L"] == 8                                 # runs are cut: combine is exercised
    assert msm(eng, ks, encs, 255, BUCKETS) == want, name
    assert msm(eng, ks, encs, 255, LANES) == want, name


@pytest.mark.parametrize("n", [0, 1, 16, 17, 4097])
def test_g2_point_sum_from_both_encodings(eng, n):
    w = world()
    want = model.mul((n * A0 + D * (n * (n - 1) // 2)) % R, G) if n else INF
    got = []
    for width, encs in ((192, w["enc"][:n]), (96, [model.encode96(p) for p in w["pts"][:n]])):
        t = dev_rows(eng, encs, width) if n else empty_rows(eng, width)
        out, finite, invalid = eng.bls12_381_g2_point_sum(t, want_invalid=True)
        got.append((bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())))
        assert got[-1] == sum_result(want), (n, width)
    assert got[0] == got[1]                                                                          # compressed and uncompressed inputs: the same bytes


def test_g2_point_sum_counts_malformed_lanes(eng):
    w, fx = world(), fixture()
    n = 300
    for width, key, enc in ((192, "malformed_uncompressed", model.encode192), (96, "malformed_compressed", model.encode96)):
        encs = [enc(p) for p in w["pts"][:n]]
        bad = [bytes.fromhex(m["bytes"]) for m in fx[key]][:17]
        for j, b in enumerate(bad):
            encs[3 + 17 * j] = b
        encs[299] = enc(INF)
        keep = [i for i in range(n) if i != 299 and not (i >= 3 and (i - 3) % 17 == 0 and (i - 3) // 17 < len(bad))]
        want = model.mul(sum(A0 + i * D for i in keep) % R, G)
        out, finite, invalid = eng.bls12_381_g2_point_sum(dev_rows(eng, encs, width), want_invalid=True)
        assert (bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())) == sum_result(want, len(bad)), width


# ---- call hygiene
def test_bad_arguments_are_refused_with_a_message_and_unaligned_arrays_work(eng):
    import ctypes as C
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    w = world()
    lib, ctx = eng.lib, eng.ctx
    k, pts = dev_scalars(eng, w["k"][:17]), dev_rows(eng, w["enc"][:17], 192)
    out = torch.full((192,), 0x5a, dtype=torch.uint8, device=eng.tdev)
    fin = torch.full((4,), 0x5a, dtype=torch.uint8, device=eng.tdev)
    inv = torch.zeros((2,), dtype=torch.int32, device=eng.tdev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda kp, pp, op, fp, ip, n, bits, flags: lib.ecsimd_bls381_g2_msm(ctx, kp, pp, op, fp, ip, C.c_size_t(n), C.c_int(bits), C.c_int(flags))
    null = C.c_void_p(0)
    for args, word in (((null, p(pts), p(out), p(fin), null, 17, 255, 1), "null"), ((p(k), null, p(out), p(fin), null, 17, 255, 1), "null"),
                       ((p(k), p(pts), null, p(fin), null, 17, 255, 1), "null"), ((p(k), p(pts), p(out), null, null, 17, 255, 1), "null"),
                       ((p(k), p(pts), p(pts), p(fin), null, 17, 255, 1), "overlap"), ((p(k), p(pts), p(out), p(out), null, 17, 255, 1), "overlap"),
                       ((p(k), p(pts), p(out), p(fin), null, 17, 0, 1), "bits"), ((p(k), p(pts), p(out), p(fin), null, 17, 257, 1), "bits"),
                       ((p(k), p(pts), p(out), p(fin), null, 17, 255, 3), "flags"), ((p(k), p(pts), p(out), p(fin), null, 17, 255, -1), "flags"),
                       ((C.c_void_p(k.data_ptr() + 8), p(pts), p(out), p(fin), null, 16, 255, 1), "aligned"),
                       ((p(k), p(pts), p(out), p(fin), C.c_void_p(inv.data_ptr() + 2), 17, 255, 1), "aligned"),
                       ((p(k), p(pts), p(out), p(fin), null, (1 << 24) + 1, 255, 1), "ECSIMD_MSM_MAX_N")):
        assert call(*args) == -1 and word in lib.ecsimd_hip_last_error(ctx).decode(), (word, lib.ecsimd_hip_last_error(ctx).decode())
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == b"\x5a" * 192 and bytes(fin.cpu().numpy()) == b"\x5a" * 4    # nothing was enqueued
    with pytest.raises(EcsimdHipError):
        eng.bls12_381_g2_raw(11, dev_rows(eng, [bytes(96)], 96))
    assert lib.ecsimd_bls381_g2_point_sum(ctx, p(pts), p(out), p(fin), null, C.c_size_t(17), C.c_int(2)) == -1 and "flags" in lib.ecsimd_hip_last_error(ctx).decode()
    assert lib.ecsimd_bls381_g2_point_sum(ctx, null, p(out), p(fin), null, C.c_size_t(17), C.c_int(0)) == -1 and "null" in lib.ecsimd_hip_last_error(ctx).decode()
    assert lib.ecsimd_bls381_g2_decompress(ctx, p(pts), p(pts), p(fin), C.c_size_t(2)) == -1 and "overlap" in lib.ecsimd_hip_last_error(ctx).decode()
    assert lib.ecsimd_bls381_g2_mul(ctx, C.c_void_p(k.data_ptr() + 8), p(pts), p(out), p(fin), C.c_size_t(1)) == -1 and "aligned" in lib.ecsimd_hip_last_error(ctx).decode()
    assert lib.ecsimd_bls381_g2_check(ctx, null, p(out), p(fin), C.c_size_t(1)) == -1 and "null" in lib.ecsimd_hip_last_error(ctx).decode()
    for fn, width in ((eng.bls12_381_g2_decompress, 96), (eng.bls12_381_g2_compress, 192), (eng.bls12_381_g2_check, 192)):   # empty batches
        a, b = fn(empty_rows(eng, width))
        assert a.shape[0] == 0 and b.shape[0] == 0
    a, b = eng.bls12_381_g2_mul(dev_scalars(eng, [1])[:0], empty_rows(eng, 192))
    assert a.shape[0] == 0 and b.shape[0] == 0
    # byte arrays at offsets 1 and 3 modulo 4, in and out
    n = 33
    encs, ks = w["enc"][:n], w["k"][:n]
    pts1 = at_offset(eng, encs, 192)
    c1, ok = eng.bls12_381_g2_compress(pts1)
    assert host_rows(c1) == [model.encode96(q) for q in w["pts"][:n]]
    u1, ok = eng.bls12_381_g2_decompress(at_offset(eng, host_rows(c1), 96, 3))
    assert host_rows(u1) == encs
    want = sum_result(expected_sum(ks, 255))
    for alg in (BUCKETS, LANES):
        o, f = eng.bls12_381_g2_msm(dev_scalars(eng, ks), at_offset(eng, encs, 192, 3 if alg == LANES else 1), bits=255, alg=alg)
        assert (bytes(o.cpu().numpy()), int(f.item()), 0) == want
    o, f = eng.bls12_381_g2_point_sum(at_offset(eng, host_rows(c1), 96, 1))
    assert bytes(o.cpu().numpy()) == model.encode192(model.mul((n * A0 + D * (n * (n - 1) // 2)) % R, G))
    for offset in (1, 3):
        outbuf = torch.zeros(192 * n + 8, dtype=torch.uint8, device=eng.tdev)
        okbuf = torch.zeros(n, dtype=torch.uint8, device=eng.tdev)
        assert lib.ecsimd_bls381_g2_mul(ctx, p(dev_scalars(eng, [1] * n)), p(pts1), C.c_void_p(outbuf.data_ptr() + offset), p(okbuf), C.c_size_t(n)) == 0
        assert bytes(outbuf[offset:offset + 192 * n].cpu().numpy()) == b"".join(encs)
    sumbuf = torch.zeros(200, dtype=torch.uint8, device=eng.tdev)                                   # the sum's result at offset 3
    assert lib.ecsimd_bls381_g2_msm(ctx, p(dev_scalars(eng, ks)), p(pts1), C.c_void_p(sumbuf.data_ptr() + 3), p(fin), null, C.c_size_t(n), C.c_int(255), C.c_int(1)) == 0
    assert bytes(sumbuf[3:195].cpu().numpy()) == want[0]


# ---- capture
def test_capture_is_refused_before_the_warm_up_and_replays_after_it():
    import torch
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    w = world()
    n = 257
    sets = [(w["k"][s:s + n], w["enc"][s:s + n], sum_result(expected_sum(w["k"][s:s + n], 255, range(s, s + n)))) for s in (0, 100, 1000)]
    eng = Engine(0)
    try:
        k, pts = dev_scalars(eng, sets[0][0]), dev_rows(eng, sets[0][1], 192)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g0, stream=side):
                try:
                    eng.bls12_381_g2_msm(k, pts, bits=255, alg=BUCKETS); said = "it did not refuse"
                except EcsimdHipError as e:
                    said = str(e)
                marker = k + 1                                                        # the capture is still valid: this node is recorded
        torch.cuda.synchronize()
        assert "(-1)" in said and "capture" in said, said
        g0.replay(); torch.cuda.synchronize()
        assert torch.equal(marker, k + 1)
        del g0
        eng.bls12_381_g2_msm(k, pts, bits=255, alg=BUCKETS); torch.cuda.synchronize()  # the warm-up at the capture's (n, bits, flags)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out, finite, invalid = eng.bls12_381_g2_msm(k, pts, bits=255, alg=BUCKETS, want_invalid=True)
        torch.cuda.synchronize()
        for ks, encs, want in sets[1:]:
            k.copy_(dev_scalars(eng, ks)); pts.copy_(dev_rows(eng, encs, 192)); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert (bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())) == want
        del g
    finally:
        eng.close()
