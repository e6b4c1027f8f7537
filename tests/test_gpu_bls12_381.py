"""GPU suite for BLS12-381 G1 (include/ecsimd_bls12_381.h).  Every expected value comes from tools/bls12_381_model.py (Python integers, the affine textbook law)
or from tests/golden/bls12_381_vectors.json, which that model writes; never from the library.  Layer by layer through ecsimd_bls12_381_raw -- the field against
Python integers on the representation's bounds, the group law on every exceptional pair --, then the encodings with every kind of malformed record, the subgroup
test against [r] P = infinity, the scalar product with integer semantics, the sum on both routes (the same bytes from each) with the batches that cut runs, fire
the doubling branch inside the buckets and sum buckets to infinity, the point sum from both encodings, call hygiene, and graph capture.

MSM terms are P_i = (a0 + i d) G, built with one affine addition per term, so an expected sum is ONE scalar product: (sum k_i (a0 + i d) mod r) G."""
import functools
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_381_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
P, R, G, INF = model.P, model.R, model.G, model.INF
OP = dict(FE_MUL=0, FE_SQR=1, FE_ADD=2, FE_SUB=3, FE_NEG=4, FE_INVERT=5, FE_SQRT=6, FE_CANON=7, POINT_ADD=8, POINT_DBL=9, POINT_MADD=10)
ALL = 2**384 - 1
AUTO, BUCKETS, LANES = 0, 1, 2
i2b = lambda v: v.to_bytes(48, "big")
b2i = lambda b: int.from_bytes(b, "big")
NMAX = 4097
A0, D = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcdef % R, 0x0fedcba987654321fedcba987654321fedcba987654321fedcba987654321 % R


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
    return dict(pts=pts, enc=[model.encode96(p) for p in pts], k=[rng.getrandbits(256) for _ in range(NMAX)])


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


def raw(engine, op, *columns):
    n = len(columns[0])
    rec = [b"".join(i2b(c[i]) for c in columns) for i in range(n)]
    out = host_rows(engine.bls12_381_raw(OP[op], dev_rows(engine, rec, 48 * len(columns))))
    return [[b2i(o[k:k + 48]) for k in range(0, len(o), 48)] for o in out]


def pt3(pt):
    return [0, 0, 1] if pt is INF else [pt[0], pt[1], 0]


def msm(engine, ks, encs, bits=255, alg=BUCKETS):
    out, finite, invalid = engine.bls12_381_g1_msm(dev_scalars(engine, ks), dev_rows(engine, encs, 96) if encs else dev_rows(engine, [bytes(96)], 96)[:0], bits=bits, alg=alg,
                                                    want_invalid=True)
    return bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())


def sum_result(pt, invalid=0):
    return (model.encode96(pt), 0 if pt is INF else 1, invalid)


# ---- the field, through raw
def test_the_field_equals_python_integers_on_random_operands_and_the_bounds(eng):
    rng = random.Random(1)
    bounds = [int(v, 16) for v in fixture()["field_operands"]]
    for want in (0, 1, P - 1, P, ALL):
        assert want in bounds
    a = [rng.getrandbits(384) for _ in range(256)] + [x for x in bounds for _ in bounds]
    b = [rng.getrandbits(384) for _ in range(256)] + [y for _ in bounds for y in bounds]
    assert raw(eng, "FE_MUL", a, b) == [[x * y % P] for x, y in zip(a, b)]
    assert raw(eng, "FE_ADD", a, b) == [[(x + y) % P] for x, y in zip(a, b)]
    assert raw(eng, "FE_SUB", a, b) == [[(x - y) % P] for x, y in zip(a, b)]
    one = a[:256] + bounds
    assert raw(eng, "FE_SQR", one) == [[x * x % P] for x in one]
    assert raw(eng, "FE_NEG", one) == [[-x % P] for x in one]
    assert raw(eng, "FE_CANON", one) == [[x % P] for x in one]


def test_inversion_and_square_roots(eng):
    rng = random.Random(2)
    a = [0, P, 1, P - 1, ALL] + [rng.getrandbits(384) for _ in range(59)]
    assert raw(eng, "FE_INVERT", a) == [[pow(x, P - 2, P)] for x in a]                             # 0 and p -> 0
    squares = [pow(rng.randrange(P), 2, P) for _ in range(24)]
    others = [(-s) % P for s in squares if s]                                                     # p = 3 mod 4: -1 is no square
    vals = [0, 1, 4, P + 4] + squares + others
    got = raw(eng, "FE_SQRT", vals)
    for v, (root, flag) in zip(vals, got):
        assert flag == (1 if model.fe_sqrt(v) is not None else 0), hex(v)
        assert root == pow(v, (P + 1) // 4, P) and (not flag or root * root % P == v % P)
    assert sum(f for _, f in got) == 4 + len(squares)


# ---- the group law, through raw
def test_the_group_law_on_every_kind_of_pair(eng):
    w = world()["pts"]
    off = model.decode96(bytes.fromhex(fixture()["off_subgroup"][0]["uncompressed"]))
    pts = [INF, G, model.neg(G), w[0], w[1], model.neg(w[1]), model.add(G, G), off, model.neg(off)]
    pairs = [(a, b) for a in pts for b in pts]                                                    # generic, P + P, P + (-P), inf + P, P + inf, inf + inf
    cols = list(zip(*[pt3(a) + pt3(b) for a, b in pairs]))
    assert raw(eng, "POINT_ADD", *cols) == [pt3(model.add(a, b)) for a, b in pairs]
    cols = list(zip(*[pt3(a) for a in pts]))
    assert raw(eng, "POINT_DBL", *cols) == [pt3(model.add(a, a)) for a in pts]
    mixed = [(a, b) for a in pts for b in pts if b is not INF]                                    # the accumulator equal to the term and to its negative among them
    cols = list(zip(*[pt3(a) + list(b) for a, b in mixed]))
    assert raw(eng, "POINT_MADD", *cols) == [pt3(model.add(a, b)) for a, b in mixed]
    assert any(a == b for a, b in mixed) and any(a is not INF and a == model.neg(b) for a, b in mixed)


# ---- the encodings
def test_the_fixture_round_trips_bit_for_bit_and_malformed_records_are_refused(eng):
    fx = fixture()
    recs = fx["multiples"] + fx["off_subgroup"] + [fx["h_torsion"]]
    u, c = [bytes.fromhex(r["uncompressed"]) for r in recs], [bytes.fromhex(r["compressed"]) for r in recs]
    assert u[0][0] == 0x40 and c[0][0] == 0xc0 and {x[0] & 0x20 for x in c[1:]} == {0, 0x20}       # infinity in both forms, both signs of y
    bad_u, bad_c = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"]], [bytes.fromhex(m["bytes"]) for m in fx["malformed_compressed"]]
    out, ok = eng.bls12_381_g1_decompress(dev_rows(eng, c + bad_c, 48))
    assert host_rows(out) == u + [bytes(96)] * len(bad_c) and ok.cpu().tolist() == [1] * len(c) + [0] * len(bad_c)
    out, ok = eng.bls12_381_g1_compress(dev_rows(eng, u + bad_u, 96))
    assert host_rows(out) == c + [bytes(48)] * len(bad_u) and ok.cpu().tolist() == [1] * len(u) + [0] * len(bad_u)
    w = world()
    out, ok = eng.bls12_381_g1_compress(dev_rows(eng, w["enc"][:300], 96))                        # more than one block
    assert host_rows(out) == [model.encode48(p) for p in w["pts"][:300]] and ok.cpu().tolist() == [1] * 300
    back, ok = eng.bls12_381_g1_decompress(out)
    assert host_rows(back) == w["enc"][:300] and ok.cpu().tolist() == [1] * 300


def test_g1_check_is_the_definition(eng):
    fx = fixture()
    recs = fx["multiples"] + fx["off_subgroup"] + [fx["h_torsion"]]
    bad = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"]]
    on, sub = eng.bls12_381_g1_check(dev_rows(eng, [bytes.fromhex(r["uncompressed"]) for r in recs] + bad, 96))
    want = [model.in_subgroup(model.decode96(bytes.fromhex(r["uncompressed"]))) for r in recs]
    assert want == [r["in_subgroup"] for r in recs] and want.count(False) >= 5 and want[0] is True   # infinity is in the subgroup
    assert on.cpu().tolist() == [1] * len(recs) + [0] * len(bad) and sub.cpu().tolist() == [int(x) for x in want] + [0] * len(bad)


def test_g1_mul_has_integer_semantics(eng):
    rng = random.Random(3)
    w = world()
    off = model.decode96(bytes.fromhex(fixture()["off_subgroup"][1]["uncompressed"]))
    ks = [0, 1, 2, R - 1, R, R + 1, 2**256 - 1] + [rng.getrandbits(256) for _ in range(64)]
    pts = [w["pts"][i] for i in range(len(ks))] + [off] * 8 + [INF]
    ks = ks + [0, 1, 2, R - 1, R, R + 1, 2**256 - 1, rng.getrandbits(256), 5]
    encs = [model.encode96(p) for p in pts] + [bytes.fromhex(fixture()["malformed_uncompressed"][0]["bytes"])]
    out, ok = eng.bls12_381_g1_mul(dev_scalars(eng, ks + [7]), dev_rows(eng, encs, 96))
    assert host_rows(out) == [model.encode96(model.mul(k, p)) for k, p in zip(ks, pts)] + [bytes(96)] and ok.cpu().tolist() == [1] * len(ks) + [0]
    assert model.mul(R, off) is not INF
    kb = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in ks[:9]), dtype=np.uint8).reshape(9, 32).copy()   # Engine converts from bytes
    import torch
    out2, _ = eng.bls12_381_g1_mul(torch.from_numpy(kb).to(eng.tdev), dev_rows(eng, encs[:9], 96))
    assert host_rows(out2) == host_rows(out)[:9]


# ---- the sum
@pytest.mark.parametrize("n", [0, 1, 2, 3, 16, 17, 33, 257, 1000, 4097])
def test_g1_msm_both_routes_give_the_models_bytes(eng, n):
    w = world()
    ks = w["k"][:n]
    want = sum_result(expected_sum(ks, 255))
    assert msm(eng, ks, w["enc"][:n], 255, BUCKETS) == want
    assert msm(eng, ks, w["enc"][:n], 255, LANES) == want
    plan = eng.bls12_381_g1_msm_plan(n, 255, AUTO)
    assert plan["route"] in (BUCKETS, LANES) and msm(eng, ks, w["enc"][:n], 255, AUTO) == want    # AUTO is the route the plan names: the same bytes either way


@pytest.mark.parametrize("bits", [1, 7, 128, 256])
def test_g1_msm_reads_only_the_low_bits(eng, bits):
    w = world()
    ks = [k | (1 << 255) | (0xdead << 200) for k in w["k"][:257]]                                 # garbage in the high bits
    want = sum_result(expected_sum(ks, bits))
    assert msm(eng, ks, w["enc"][:257], bits, BUCKETS) == want and msm(eng, ks, w["enc"][:257], bits, LANES) == want


def special_batches():
    w = world()
    n = 1000
    rng = random.Random(4)
    k0 = rng.getrandbits(255)
    out = {}
    out["every scalar equal"] = ([k0] * n, w["enc"][:n], sum_result(expected_sum([k0] * n, 255)))
    out["every point equal"] = (w["k"][:n], [w["enc"][5]] * n, sum_result(model.mul(sum(k % 2**255 for k in w["k"][:n]) * (A0 + 5 * D) % R, G)))
    neg5 = model.encode96(model.neg(w["pts"][5]))
    out["alternating P and -P"] = ([k0] * n, [w["enc"][5] if i % 2 == 0 else neg5 for i in range(n)], sum_result(INF))
    out["all scalars zero"] = ([0] * n, w["enc"][:n], sum_result(INF))
    ks = list(w["k"][:n - 1]); tot = sum((k % 2**255) * (A0 + i * D) for i, k in enumerate(ks)) % R
    last = (-tot * pow(A0 + (n - 1) * D, -1, R)) % R
    assert last < 2**255
    out["a total of infinity"] = (ks + [last], w["enc"][:n], sum_result(INF))
    fx = fixture()
    bad = [bytes.fromhex(m["bytes"]) for m in fx["malformed_uncompressed"][:5]]
    offs = [model.decode96(bytes.fromhex(r["uncompressed"])) for r in fx["off_subgroup"][:2]]
    encs, ks = list(w["enc"][:n]), list(w["k"][:n])
    for j, b in enumerate(bad):
        encs[10 + 97 * j] = b
    for j in range(5):
        encs[20 + 101 * j] = model.encode96(INF)
    where_off = (333, 777)
    for j, o in zip(where_off, offs):
        encs[j] = model.encode96(o)
    skipped = {10 + 97 * j for j in range(5)} | {20 + 101 * j for j in range(5)} | set(where_off)
    idx = [i for i in range(n) if i not in skipped]
    acc = expected_sum([ks[i] for i in idx], 255, idx)
    for j, o in zip(where_off, offs):
        acc = model.add(acc, model.mul(ks[j] % 2**255, o))                                       # the sum is over the integers
    out["malformed, infinite and off-subgroup terms"] = (ks, encs, sum_result(acc, 5))
    return out


@pytest.mark.parametrize("name", ["every scalar equal", "every point equal", "alternating P and -P", "all scalars zero", "a total of infinity",
                                  "malformed, infinite and off-subgroup terms"])
def test_g1_msm_special_batches(eng, name):
    ks, encs, want = special_batches()[name]
    assert eng.bls12_381_g1_msm_plan(1000, 255, BUCKETS)["L"] == 8                                 # runs are cut: combine is exercised
    assert msm(eng, ks, encs, 255, BUCKETS) == want, name
    assert msm(eng, ks, encs, 255, LANES) == want, name


@pytest.mark.parametrize("n", [0, 1, 16, 17, 4097])
def test_g1_point_sum_from_both_encodings(eng, n):
    w = world()
    want = model.mul((n * A0 + D * (n * (n - 1) // 2)) % R, G) if n else INF
    for width, encs in ((96, w["enc"][:n]), (48, [model.encode48(p) for p in w["pts"][:n]])):
        t = dev_rows(eng, encs, width) if n else dev_rows(eng, [bytes(width)], width)[:0]
        out, finite, invalid = eng.bls12_381_g1_point_sum(t, want_invalid=True)
        assert (bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())) == sum_result(want), (n, width)


def test_g1_point_sum_counts_malformed_lanes(eng):
    w, fx = world(), fixture()
    n = 300
    for width, key, enc in ((96, "malformed_uncompressed", model.encode96), (48, "malformed_compressed", model.encode48)):
        encs = [enc(p) for p in w["pts"][:n]]
        bad = [bytes.fromhex(m["bytes"]) for m in fx[key]]
        for j, b in enumerate(bad):
            encs[3 + 17 * j] = b
        encs[299] = enc(INF)
        keep = [i for i in range(n) if i != 299 and not (i >= 3 and (i - 3) % 17 == 0 and (i - 3) // 17 < len(bad))]
        want = model.mul(sum(A0 + i * D for i in keep) % R, G)
        out, finite, invalid = eng.bls12_381_g1_point_sum(dev_rows(eng, encs, width), want_invalid=True)
        assert (bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())) == sum_result(want, len(bad)), width


# ---- call hygiene
def test_bad_arguments_are_refused_with_a_message_and_unaligned_arrays_work(eng):
    import ctypes as C
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    w = world()
    lib, ctx = eng.lib, eng.ctx
    k, pts = dev_scalars(eng, w["k"][:17]), dev_rows(eng, w["enc"][:17], 96)
    out = torch.full((96,), 0x5a, dtype=torch.uint8, device=eng.tdev)
    fin = torch.full((4,), 0x5a, dtype=torch.uint8, device=eng.tdev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda kp, pp, op, fp, ip, n, bits, flags: lib.ecsimd_bls12_381_g1_msm(ctx, kp, pp, op, fp, ip, C.c_size_t(n), C.c_int(bits), C.c_int(flags))
    null = C.c_void_p(0)
    for args, word in (((null, p(pts), p(out), p(fin), null, 17, 255, 1), "null"), ((p(k), null, p(out), p(fin), null, 17, 255, 1), "null"),
                       ((p(k), p(pts), null, p(fin), null, 17, 255, 1), "null"), ((p(k), p(pts), p(out), null, null, 17, 255, 1), "null"),
                       ((p(k), p(pts), p(pts), p(fin), null, 17, 255, 1), "overlap"), ((p(k), p(pts), p(out), p(out), null, 17, 255, 1), "overlap"),
                       ((p(k), p(pts), p(out), p(fin), null, 17, 0, 1), "bits"), ((p(k), p(pts), p(out), p(fin), null, 17, 257, 1), "bits"),
                       ((p(k), p(pts), p(out), p(fin), null, 17, 255, 3), "flags"), ((p(k), p(pts), p(out), p(fin), null, 17, 255, -1), "flags"),
                       ((C.c_void_p(k.data_ptr() + 8), p(pts), p(out), p(fin), null, 16, 255, 1), "aligned"),
                       ((p(k), p(pts), p(out), p(fin), null, (1 << 24) + 1, 255, 1), "ECSIMD_MSM_MAX_N")):
        assert call(*args) == -1 and word in lib.ecsimd_hip_last_error(ctx).decode(), (word, lib.ecsimd_hip_last_error(ctx).decode())
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == b"\x5a" * 96 and bytes(fin.cpu().numpy()) == b"\x5a" * 4     # nothing was enqueued
    with pytest.raises(EcsimdHipError):
        eng.bls12_381_raw(11, dev_rows(eng, [bytes(48)], 48))
    assert lib.ecsimd_bls12_381_g1_point_sum(ctx, p(pts), p(out), p(fin), null, C.c_size_t(17), C.c_int(2)) == -1
    assert lib.ecsimd_bls12_381_g1_decompress(ctx, p(pts), p(pts), p(fin), C.c_size_t(2)) == -1 and "overlap" in lib.ecsimd_hip_last_error(ctx).decode()
    for fn, width in ((eng.bls12_381_g1_decompress, 48), (eng.bls12_381_g1_compress, 96), (eng.bls12_381_g1_check, 96)):   # empty batches
        a, b = fn(dev_rows(eng, [bytes(width)], width)[:0])
        assert a.shape[0] == 0 and b.shape[0] == 0
    # byte arrays at offset 1
    n = 33
    encs, ks = w["enc"][:n], w["k"][:n]
    pts1 = at_offset(eng, encs, 96)
    c1, ok = eng.bls12_381_g1_compress(pts1)
    assert host_rows(c1) == [model.encode48(q) for q in w["pts"][:n]]
    u1, ok = eng.bls12_381_g1_decompress(at_offset(eng, host_rows(c1), 48, 3))
    assert host_rows(u1) == encs
    want = sum_result(expected_sum(ks, 255))
    for alg in (BUCKETS, LANES):
        o, f = eng.bls12_381_g1_msm(dev_scalars(eng, ks), pts1, bits=255, alg=alg)
        assert (bytes(o.cpu().numpy()), int(f.item()), 0) == want
    o, f = eng.bls12_381_g1_point_sum(at_offset(eng, host_rows(c1), 48, 1))
    assert bytes(o.cpu().numpy()) == model.encode96(model.mul((n * A0 + D * (n * (n - 1) // 2)) % R, G))
    outbuf = torch.zeros(96 * n + 8, dtype=torch.uint8, device=eng.tdev)
    okbuf = torch.zeros(n, dtype=torch.uint8, device=eng.tdev)
    assert lib.ecsimd_bls12_381_g1_mul(ctx, p(dev_scalars(eng, [1] * n)), p(pts1), C.c_void_p(outbuf.data_ptr() + 1), p(okbuf), C.c_size_t(n)) == 0
    assert bytes(outbuf[1:1 + 96 * n].cpu().numpy()) == b"".join(encs)


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
        k, pts = dev_scalars(eng, sets[0][0]), dev_rows(eng, sets[0][1], 96)
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g0, stream=side):
                try:
                    eng.bls12_381_g1_msm(k, pts, bits=255, alg=BUCKETS); said = "it did not refuse"
                except EcsimdHipError as e:
                    said = str(e)
                marker = k + 1                                                        # the capture is still valid: this node is recorded
        torch.cuda.synchronize()
        assert "(-1)" in said and "capture" in said, said
        g0.replay(); torch.cuda.synchronize()
        assert torch.equal(marker, k + 1)
        del g0
        eng.bls12_381_g1_msm(k, pts, bits=255, alg=BUCKETS); torch.cuda.synchronize()  # the warm-up at the capture's (n, bits, flags)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out, finite, invalid = eng.bls12_381_g1_msm(k, pts, bits=255, alg=BUCKETS, want_invalid=True)
        torch.cuda.synchronize()
        for ks, encs, want in sets[1:]:
            k.copy_(dev_scalars(eng, ks)); pts.copy_(dev_rows(eng, encs, 96)); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            assert (bytes(out.cpu().numpy()), int(finite.item()), int(invalid.item())) == want
        del g
    finally:
        eng.close()
