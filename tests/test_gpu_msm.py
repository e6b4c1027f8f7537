"""Multi-scalar multiplication on the device (include/ecsimd_msm.h): Engine.msm through all three routes and Engine.point_sum against the big-int group law of
tests/helpers.py -- term by term up to 257 terms, and through P_i = a_i G with known a_i, where the sum is (sum k_i a_i mod n) G, at every size.  The aimed
inputs are built from Engine.msm_plan's c, L and m.  In every case the three routes agree byte for byte on (rx, ry, finite), and a second call on the same
context gives the same bytes (workspace reuse, stale histograms)."""
import hashlib
import random
import time

import numpy as np
import pytest

from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add, ec_mul, ints_to_arr, arr_to_ints

pytestmark = pytest.mark.gpu
CURVES = (P256, SECP256K1)
AUTO, BUCKETS, LANES = 0, 1, 2
WALK = 4099


def G(cv):
    return (CURVE_PARAMS[cv]["gx"], CURVE_PARAMS[cv]["gy"])


def neg(cv, P):
    return (P[0], CURVE_PARAMS[cv]["p"] - P[1])


_walks = {}


def walk(cv):
    """P_i = (i + 1) G for i < 4099, by repeated addition: computed once per curve and never changed."""
    if cv not in _walks:
        P, out = G(cv), []
        for _ in range(WALK):
            out.append(P); P = ec_add(cv, P, G(cv))
        _walks[cv] = tuple(out)
    return _walks[cv]


def dev(engine, ints):
    return engine.to_device(ints_to_arr(list(ints)) if len(ints) else np.zeros((0, 4), dtype=np.uint64))


def point_of(rx, ry, finite):
    x, y = arr_to_ints(rx)[0], arr_to_ints(ry)[0]
    if not finite[0]:
        assert (x, y) == (0, 0), "an infinite result must be (0, 0)"
        return None
    return (x, y)


def run_msm(engine, cv, ks, pts, bits=256, invalid=0, algs=(BUCKETS, LANES, AUTO)):
    """Every route twice on the same context; returns the one point all of them gave."""
    import torch
    k, x, y = dev(engine, ks), dev(engine, [p[0] for p in pts]), dev(engine, [p[1] for p in pts])
    seen = {}
    for alg in algs:
        for again in (0, 1):
            rx, ry, fin, bad = engine.msm(cv, k, x, y, bits=bits, alg=alg, want_invalid=True)
            torch.cuda.synchronize()
            seen[(alg, again)] = (engine.to_numpy(rx).tobytes(), engine.to_numpy(ry).tobytes(), bytes(fin.cpu().numpy()))
            assert int(bad.cpu()[0]) == invalid, (alg, again)
    first = seen[(algs[0], 0)]
    assert all(v == first for v in seen.values()), {key: v == first for key, v in seen.items()}
    assert first[2] in (b"\x00", b"\x01")
    return point_of(np.frombuffer(first[0], dtype=np.uint64).reshape(1, 4), np.frombuffer(first[1], dtype=np.uint64).reshape(1, 4), first[2])


def via_generator(cv, ks, a, bits):
    order = CURVE_PARAMS[cv]["n"]
    return ec_mul(cv, sum((k % (1 << bits)) * ai for k, ai in zip(ks, a)) % order, G(cv))


def term_by_term(cv, ks, pts, bits):
    acc = None
    for k, P in zip(ks, pts):
        acc = ec_add(cv, acc, ec_mul(cv, k % (1 << bits), P))
    return acc


# ---- sizes
@pytest.mark.parametrize("bits", (256, 128, 1, 101))
@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65, 257, 4099))
@pytest.mark.parametrize("cv", CURVES)
def test_sizes_through_all_three_routes(engine, cv, n, bits):
    rng = random.Random(1000 * n + bits + cv)
    pts = walk(cv)[:n]
    ks = [rng.getrandbits(256) for _ in range(n)]
    if n:
        c = engine.msm_plan(n, bits, BUCKETS)["c"]
        assert bits != 101 or bits % c                                   # the bits value that is no multiple of the window width
    got = run_msm(engine, cv, ks, pts, bits)
    assert got == via_generator(cv, ks, range(1, n + 1), bits)
    if n <= 257:
        assert got == term_by_term(cv, ks, pts, bits)


# ---- aimed inputs
def fixed_points_of_L():
    from ecsimd_amd import Engine
    hit = []
    for n in range(1, 600):
        L = Engine.msm_plan(n, 256, BUCKETS)["L"]
        if n in (L - 1, L, L + 1, 2 * L + 1): hit.append(n)
    return hit


@pytest.mark.parametrize("cv", CURVES)
def test_every_scalar_and_point_equal_at_the_split_length(engine, cv):
    sizes = fixed_points_of_L()
    assert {3, 4, 5, 9} <= set(sizes)                                    # L = 4 up to 256 terms: L - 1, L, L + 1, 2 L + 1
    rng = random.Random(41 + cv)
    P = walk(cv)[rng.randrange(WALK)]
    order = CURVE_PARAMS[cv]["n"]
    for n in sizes + [8 * 4 + 1, 257, 1025, 4099]:                       # ... and runs that cross many slices at larger L
        k = rng.getrandbits(256)
        L = engine.msm_plan(n, 256, BUCKETS)["L"]
        assert n > L or n in (3, 4)
        assert run_msm(engine, cv, [k] * n, [P] * n) == ec_mul(cv, k * n % order, P), n


def test_every_scalar_equal_at_65536_terms_is_no_serial_sum(engine):
    """The serial bound on the device: one bucket per window holds all n entries; its lane combines ceil(n / L) + 1 = 1025 slice sums, no lane adds 65 536."""
    import torch
    cv, n = SECP256K1, 1 << 16
    plan = engine.msm_plan(n, 256, BUCKETS)
    assert plan["max_chain"] == n // plan["L"] + 1 <= 4 * 256 + 1
    P = walk(cv)[77]
    k = random.Random(65536).getrandbits(256)
    kd, xd, yd = (engine.to_device(np.tile(ints_to_arr([v]), (n, 1))) for v in (k, P[0], P[1]))
    out = {}
    for alg in (BUCKETS, LANES, BUCKETS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        rx, ry, fin = engine.msm(cv, kd, xd, yd, alg=alg)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print(f"all-equal msm, n = 2^16, alg = {alg}: {dt * 1e3:.2f} ms (the first call of a route also grows the workspace)")
        out[alg] = point_of(engine.to_numpy(rx), engine.to_numpy(ry), fin.cpu().numpy())
    assert out[BUCKETS] == out[LANES] == ec_mul(cv, k * n % CURVE_PARAMS[cv]["n"], P)


@pytest.mark.parametrize("cv", CURVES)
def test_cancelling_terms(engine, cv):
    rng = random.Random(7 + cv)
    order = CURVE_PARAMS[cv]["n"]
    pts = list(walk(cv)[100:140])
    ks = [rng.getrandbits(256) for _ in pts]
    # (k, P) and (k, -P): every bucket sums to infinity; one more term so that something is left
    assert run_msm(engine, cv, ks + ks + [5], pts + [neg(cv, Q) for Q in pts] + [pts[0]]) == ec_mul(cv, 5, pts[0])
    assert run_msm(engine, cv, ks + ks, pts + [neg(cv, Q) for Q in pts]) is None
    # (k, P) and (n - k, P): the buckets differ, the total is infinity: finite = 0 and (0, 0)
    ks = [rng.randrange(1, order) for _ in pts]
    assert run_msm(engine, cv, ks + [order - k for k in ks], pts + pts) is None
    assert run_msm(engine, cv, [0] * 40, pts) is None
    assert run_msm(engine, cv, ks, [(0, 0)] * 40) is None


@pytest.mark.parametrize("cv", CURVES)
def test_full_digits_and_single_windows(engine, cv):
    n = 70
    pts, a = walk(cv)[:n], range(1, n + 1)
    for bits in (256, 128, 101):                                         # k = 2^bits - 1: the top digit is full in every window
        assert run_msm(engine, cv, [(1 << 256) - 1] * n, pts, bits) == via_generator(cv, [(1 << bits) - 1] * n, a, 256), bits
    plan = engine.msm_plan(n, 255, BUCKETS)
    c, W = plan["c"], plan["windows"]
    assert 255 % c                                                       # the top window is a partial one
    for name, k in (("lowest", (1 << c) - 1), ("highest", 1 << 254), ("partial top", ((1 << c) - 1) << (c * (W - 1))), ("below the top", ((1 << c) - 1) << (c * (W - 2)))):
        assert run_msm(engine, cv, [k] * n, pts, 255) == via_generator(cv, [k] * n, a, 255), name


@pytest.mark.parametrize("cv", CURVES)
def test_the_chunk_edges_of_the_bucket_reduction(engine, cv):
    n = WALK
    plan = engine.msm_plan(n, 16, BUCKETS)
    c, m, top = plan["c"], plan["m"], plan["buckets"] - 1
    assert plan["windows"] == 2 and top > m + 1
    edge = (m - 1, m, m + 1, top)                                        # the only buckets populated
    ks = [edge[i % 4] | (edge[(i // 4) % 4] << c) for i in range(n)]
    assert run_msm(engine, cv, ks, walk(cv), 16) == via_generator(cv, ks, range(1, n + 1), 16)


@pytest.mark.parametrize("cv", CURVES)
def test_bits_128_ignores_the_upper_half_of_every_scalar(engine, cv):
    rng = random.Random(128 + cv)
    n = 300
    low = [rng.getrandbits(128) for _ in range(n)]
    want = via_generator(cv, low, range(1, n + 1), 128)
    assert run_msm(engine, cv, low, walk(cv)[:n], 128) == want
    assert run_msm(engine, cv, [k | (rng.getrandbits(128) << 128) | (1 << 255) for k in low], walk(cv)[:n], 128) == want


@pytest.mark.parametrize("cv", CURVES)
def test_invalid_points_count_and_contribute_nothing(engine, cv):
    rng = random.Random(404 + cv)
    p = CURVE_PARAMS[cv]["p"]
    n = 90
    pts = list(walk(cv)[:n]); ks = [rng.getrandbits(256) for _ in range(n)]
    bad = {3: (pts[3][0], (pts[3][1] + 1) % p),                          # off the curve
           17: (p, pts[17][1]),                                          # x = p
           40: (pts[40][0], p), 41: (pts[41][0], (1 << 256) - 1),        # y >= p
           89: (pts[89][1], pts[89][0])}                                 # off the curve, last lane
    dirty = [bad.get(i, P) for i, P in enumerate(pts)]
    clean = [(0, 0) if i in bad else P for i, P in enumerate(pts)]
    want = run_msm(engine, cv, ks, clean)
    assert want == via_generator(cv, [0 if i in bad else k for i, k in enumerate(ks)], range(1, n + 1), 256)
    assert run_msm(engine, cv, ks, dirty, invalid=len(bad)) == want


# ---- point_sum
def run_point_sum(engine, cv, pts, invalid=0):
    import torch
    x, y = dev(engine, [p[0] for p in pts]), dev(engine, [p[1] for p in pts])
    seen = []
    for _ in range(2):
        rx, ry, fin, bad = engine.point_sum(cv, x, y, want_invalid=True)
        torch.cuda.synchronize()
        seen.append((engine.to_numpy(rx).tobytes(), engine.to_numpy(ry).tobytes(), bytes(fin.cpu().numpy())))
        assert int(bad.cpu()[0]) == invalid
    assert seen[0] == seen[1]
    return point_of(engine.to_numpy(rx), engine.to_numpy(ry), fin.cpu().numpy())


@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257, 4099))
@pytest.mark.parametrize("cv", CURVES)
def test_point_sum_sizes(engine, cv, n):
    order = CURVE_PARAMS[cv]["n"]
    assert run_point_sum(engine, cv, walk(cv)[:n]) == ec_mul(cv, n * (n + 1) // 2 % order, G(cv))


@pytest.mark.parametrize("cv", CURVES)
def test_point_sum_of_equal_opposite_infinite_and_invalid_points(engine, cv):
    p, order = CURVE_PARAMS[cv]["p"], CURVE_PARAMS[cv]["n"]
    P = walk(cv)[10]
    for n in (2, 16, 17, 257, 1000):                                     # all points equal: the tangent at every level of the tree
        assert run_point_sum(engine, cv, [P] * n) == ec_mul(cv, n % order, P), n
    for n in (2, 33, 256, 513):                                          # P, -P, P, ...
        assert run_point_sum(engine, cv, [P if i % 2 == 0 else neg(cv, P) for i in range(n)]) == (P if n % 2 else None), n
    pts = [(0, 0) if i % 3 == 0 else Q for i, Q in enumerate(walk(cv)[:300])]
    assert run_point_sum(engine, cv, pts) == ec_mul(cv, sum(i + 1 for i in range(300) if i % 3) % order, G(cv))
    assert run_point_sum(engine, cv, [(0, 0)] * 40) is None
    pts[1] = (pts[1][0], pts[1][1] ^ 1); pts[299] = (p, 5)
    assert run_point_sum(engine, cv, pts, invalid=2) == ec_mul(cv, sum(i + 1 for i in range(300) if i % 3 and i not in (1, 299)) % order, G(cv))


# ---- BIP-340 batch verification as ONE msm
def lift_x(x):
    p = CURVE_PARAMS[SECP256K1]["p"]
    y = pow((x * x * x + 7) % p, (p + 1) // 4, p)
    assert y * y % p == (x * x * x + 7) % p
    return (x, y if y % 2 == 0 else p - y)


def challenge(r, px, msg):
    tag = hashlib.sha256(b"BIP0340/challenge").digest()
    return int.from_bytes(hashlib.sha256(tag + tag + r.to_bytes(32, "big") + px.to_bytes(32, "big") + msg).digest(), "big") % CURVE_PARAMS[SECP256K1]["n"]


def test_bip340_batch_verification_is_one_msm(engine):
    import torch
    cv, u = SECP256K1, 64
    order = CURVE_PARAMS[cv]["n"]
    rng = random.Random(340)
    d = [rng.randrange(1, order) for _ in range(u)]
    msgs = [rng.randbytes(32) for _ in range(u)]
    px, r, s, ok = engine.schnorr_sign(dev(engine, d), torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(u, 32).copy()).to(engine.tdev))
    torch.cuda.synchronize()
    assert ok.cpu().numpy().all()
    px, r, s = (arr_to_ints(engine.to_numpy(t)) for t in (px, r, s))
    a = [1] + [rng.getrandbits(128) for _ in range(u - 1)]                # BIP-340 "Batch Verification": a_0 = 1, the others 128-bit
    e = [challenge(r[i], px[i], msgs[i]) for i in range(u)]

    def terms(svals):
        ks = [(-sum(ai * si for ai, si in zip(a, svals))) % order] + a + [ai * ei % order for ai, ei in zip(a, e)]
        return ks, [G(cv)] + [lift_x(v) for v in r] + [lift_x(v) for v in px]

    ks, pts = terms(s)
    assert len(ks) == 129
    assert run_msm(engine, cv, ks, pts) is None                           # (s_0 + a_1 s_1 + ...) G = R_0 + a_1 R_1 + ... + e_0 P_0 + (a_1 e_1) P_1 + ...
    forged = list(s); forged[37] ^= 1 << 100
    ks, pts = terms(forged)
    assert run_msm(engine, cv, ks, pts) == ec_mul(cv, (-a[37] * (forged[37] - s[37])) % order, G(cv))      # a finite point: the batch is refused


# ---- stream capture
def captured(eng, fn):
    import torch
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fn()
    torch.cuda.synchronize()                                             # the capture ended without error
    return g, out


def test_a_captured_msm_replays_to_the_eager_result():
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    try:
        cv, n = P256, 257
        rng = random.Random(257)
        pts = walk(cv)[:n]
        sets = [[rng.getrandbits(256) for _ in range(n)] for _ in range(3)]
        k, x, y = dev(eng, sets[0]), dev(eng, [p[0] for p in pts]), dev(eng, [p[1] for p in pts])
        for alg in (BUCKETS, LANES):
            eng.msm(cv, k, x, y, alg=alg, want_invalid=True)             # the warm-up at the capture's (n, bits, flags)
        torch.cuda.synchronize()
        g, out = captured(eng, lambda: {alg: eng.msm(cv, k, x, y, alg=alg, want_invalid=True) for alg in (BUCKETS, LANES)})
        for i in (1, 2):
            k.copy_(dev(eng, sets[i])); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            got = {alg: tuple(t.clone() for t in out[alg]) for alg in out}
            want = via_generator(cv, sets[i], range(1, n + 1), 256)
            for alg in (BUCKETS, LANES):
                eager = eng.msm(cv, k, x, y, alg=alg, want_invalid=True); torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(got[alg], eager)), (alg, i)
                assert int(got[alg][3].cpu()[0]) == 0
                assert point_of(eng.to_numpy(got[alg][0]), eng.to_numpy(got[alg][1]), got[alg][2].cpu().numpy()) == want, (alg, i)
        del out, g
    finally:
        eng.close()


def test_a_capture_without_a_warm_up_is_refused_and_stays_valid():
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    eng = Engine(0)
    try:
        cv, n, big = P256, 257, 20000
        pts = walk(cv)[:n]
        ks = [random.Random(258).getrandbits(256) for _ in range(n)]
        k, x, y = dev(eng, ks), dev(eng, [p[0] for p in pts]), dev(eng, [p[1] for p in pts])
        kb, xb, yb = (eng.to_device(np.tile(ints_to_arr([v]), (big, 1))) for v in (3, pts[0][0], pts[0][1]))
        eng.msm(cv, k, x, y, alg=BUCKETS); torch.cuda.synchronize()      # the small batch is warmed up, the large one is not
        said = {}

        def body():
            for alg in (BUCKETS, LANES):                                 # the workspace would have to grow
                try:
                    eng.msm(cv, kb, xb, yb, alg=alg)
                    said[alg] = "it did not refuse"
                except EcsimdHipError as exc:
                    said[alg] = str(exc)
            return eng.msm(cv, k, x, y, alg=BUCKETS)
        g, out = captured(eng, body)
        assert all("capture" in msg and "(-1)" in msg for msg in said.values()), said
        g.replay(); torch.cuda.synchronize()
        assert point_of(eng.to_numpy(out[0]), eng.to_numpy(out[1]), out[2].cpu().numpy()) == via_generator(cv, ks, range(1, n + 1), 256)
        del out, g
        rx, ry, fin = eng.msm(cv, kb, xb, yb, alg=BUCKETS); torch.cuda.synchronize()      # outside a capture the larger batch runs
        assert point_of(eng.to_numpy(rx), eng.to_numpy(ry), fin.cpu().numpy()) == ec_mul(cv, 3 * big, pts[0])
    finally:
        eng.close()


# ---- refusals
def test_bad_arguments_are_refused(engine):
    from ecsimd_amd import EcsimdHipError
    cv = P256
    k, x, y = dev(engine, [1, 2]), dev(engine, [p[0] for p in walk(cv)[:2]]), dev(engine, [p[1] for p in walk(cv)[:2]])
    for kwargs in (dict(bits=0), dict(bits=257), dict(alg=3), dict(alg=4), dict(alg=-1)):
        with pytest.raises(EcsimdHipError):
            engine.msm(cv, k, x, y, **kwargs)
    with pytest.raises(EcsimdHipError, match="registered curves have no multi-scalar multiplication"):
        engine.msm(0x10000, k, x, y)
    with pytest.raises(EcsimdHipError, match="registered curves"):
        engine.point_sum(0x10000, x, y)
    with pytest.raises(EcsimdHipError):
        engine.msm(7, k, x, y)
    assert run_msm(engine, cv, [1, 2], walk(cv)[:2]) == ec_mul(cv, 5, G(cv))      # the context still works
