"""The schedule of the multi-scalar multiplication (include/ecsimd_msm.h; k_msm.inc, msm_schedule_of in capi.hip) on the device, at the (n, bits) that
tests/test_gpu_msm.py does not reach: every window width c = 1 .. 16 on populated buckets, the tree over the windows at depths 1, 2 and 3, AUTO on both sides of
its threshold, one-hot scalars in the windows that straddle a 32-bit word, every layout of a bucket over the slices, LANES across a chunk of the per-lane product,
and operands nobody had passed.  tests/msm_cases.py makes the inputs; tests/test_msm_cases_cpu.py holds them to their conditions without a GPU.

The expected value is always the big-int group law of tests/helpers.py -- where P_i = a_i G, (sum (k_i mod 2^bits) a_i mod order) G -- never another route of the
device and never tools/msm_model.py.  In every case BUCKETS runs twice on one context and must give the same bytes; LANES and AUTO run where stated and must agree
with them; invalid == 0 unless the case is about invalid points."""
import ctypes as C
import random

import numpy as np
import pytest

import msm_cases as cases
import msm_model as model
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add, ec_mul

pytestmark = pytest.mark.gpu
CURVES = cases.CURVES
AUTO, BUCKETS, LANES = cases.AUTO, cases.BUCKETS, cases.LANES
OUT_AFFINE = 2
G, walk = cases.G, cases.walk


def neg(cv, P):
    return (P[0], CURVE_PARAMS[cv]["p"] - P[1])


def call(engine, cv, k, x, y, bits, alg, invalid=0):
    """One ecsimd_msm: the result's bytes (rx, ry, finite)."""
    import torch
    rx, ry, fin, bad = engine.msm(cv, k, x, y, bits=bits, alg=alg, want_invalid=True)
    torch.cuda.synchronize()
    assert int(bad.cpu()[0]) == invalid, (alg, int(bad.cpu()[0]))
    return engine.to_numpy(rx).tobytes(), engine.to_numpy(ry).tobytes(), bytes(fin.cpu().numpy())


def point_of(triple):
    x, y = (int.from_bytes(b, "little") for b in triple[:2])
    assert triple[2] in (b"\x00", b"\x01")
    if triple[2] == b"\x00":
        assert (x, y) == (0, 0), "an infinite result must be (0, 0)"
        return None
    return (x, y)


def run(engine, cv, k, x, y, bits=256, others=(LANES, AUTO), invalid=0):
    """BUCKETS twice on the same context, then the other routes once: all the same bytes.  Returns the point."""
    first = call(engine, cv, k, x, y, bits, BUCKETS, invalid)
    assert call(engine, cv, k, x, y, bits, BUCKETS, invalid) == first, "BUCKETS a second time on the same context"
    for alg in others:
        assert call(engine, cv, k, x, y, bits, alg, invalid) == first, alg
    return point_of(first)


def run_ints(engine, cv, ks, pts, bits=256, others=(LANES, AUTO), invalid=0):
    k, x, y = (engine.to_device(cases.limbs_of(v)) for v in (ks, [p[0] for p in pts], [p[1] for p in pts]))
    return run(engine, cv, k, x, y, bits, others, invalid)


def term_by_term(cv, ks, pts, bits=256):
    acc = None
    for k, P in zip(ks, pts):
        acc = ec_add(cv, acc, ec_mul(cv, k % (1 << bits), P))
    return acc


_walk_dev = {}


def walk_on_device(engine, cv, n):
    """(x, y) of walk(cv)[i mod 4099] for i < n, indexed on the device: no host array of n points."""
    import torch
    if cv not in _walk_dev:                                               # torch's tensors on device 0: every context of these tests may read them
        _walk_dev[cv] = tuple(engine.to_device(cases.limbs_of([p[j] for p in walk(cv)])) for j in (0, 1))
    wx, wy = _walk_dev[cv]
    if n <= cases.WALK: return wx[:n].contiguous(), wy[:n].contiguous()
    idx = torch.arange(n, device=engine.tdev) % cases.WALK
    return wx[idx].contiguous(), wy[idx].contiguous()


def walk_dot(ks, bits, order):
    return sum((k % (1 << bits)) * (i % cases.WALK + 1) for i, k in enumerate(ks)) % order


# ---- 1. every window width on populated buckets
def test_the_width_cases_reach_every_c_and_every_tree_depth(engine):
    seen_c, seen_depth = set(), set()
    for c, n, bits in cases.WIDTH_CASES + cases.PARTIAL_TOP_CASES:
        plan = engine.msm_plan(n, bits, BUCKETS)
        seen_c.add(plan["c"]); seen_depth.add(cases.tree_passes(plan))
    assert seen_c == set(range(1, 17)) and {1, 2, 3} <= seen_depth, (seen_c, seen_depth)


@pytest.mark.parametrize("case", cases.WIDTH_CASES + cases.PARTIAL_TOP_CASES, ids=cases.width_case_id)
@pytest.mark.parametrize("cv", CURVES)
def test_every_window_width(engine, cv, case):
    import torch
    c, n, bits = case
    order = CURVE_PARAMS[cv]["n"]
    plan = engine.msm_plan(n, bits, BUCKETS)
    assert plan["c"] == c
    assert plan == model.plan(n, bits, BUCKETS)
    for row in cases.WIDTH_TABLE:
        if row[:2] == (c, n) and bits == 256:
            assert (plan["c"], n, plan["windows"], plan["m"], plan["L"], plan["buckets"] // plan["m"], cases.tree_passes(plan)) == row
    a, k = cases.width_batch(cv, n, bits)
    al = np.zeros((n, 4), dtype=np.uint64); al[:, 0] = a
    x, y = engine.scalar_mult_base(cv, engine.to_device(al), OUT_AFFINE)
    torch.cuda.synchronize()
    lanes = np.random.default_rng([cv, n, bits]).choice(n, size=min(n, cases.SPOT_LANES), replace=False)
    lanes.sort()
    sx, sy = (cases.ints_of(engine.to_numpy(engine.select_rows(t, lanes))) for t in (x, y))
    for j, i in enumerate(lanes):                                        # the points are what the reference takes them to be
        assert (sx[j], sy[j]) == ec_mul(cv, int(a[i]), G(cv)), i
    kd = engine.to_device(k)
    total = cases.dot_mod(k, a, bits, order)
    got = run(engine, cv, kd, x, y, bits, others=(LANES,) if n <= cases.LANES_MAX_N else ())
    assert got == ec_mul(cv, total, G(cv)), (c, n, bits)
    if n == model.AUTO_THRESHOLD:
        assert engine.msm_plan(n, bits, AUTO)["route"] == BUCKETS and engine.msm_plan(n - 1, bits, AUTO)["route"] == LANES
        assert point_of(call(engine, cv, kd, x, y, bits, AUTO)) == got                                     # (run compared LANES; this is AUTO = BUCKETS, byte for byte)
        assert call(engine, cv, kd, x, y, bits, AUTO) == call(engine, cv, kd, x, y, bits, BUCKETS)
        last = int(cases.ints_of(cases.mask_limbs(k[n - 1:], bits))[0]) * int(a[n - 1])
        below = call(engine, cv, kd[:n - 1], x[:n - 1], y[:n - 1], bits, AUTO)
        assert point_of(below) == ec_mul(cv, (total - last) % order, G(cv))


# ---- 2. one-hot windows at the word boundaries
@pytest.mark.parametrize("bits", cases.ONE_HOT_BITS)
@pytest.mark.parametrize("c", cases.ONE_HOT_WIDTHS)
@pytest.mark.parametrize("cv", CURVES)
def test_single_window_scalars_at_straddling_widths(engine, cv, c, bits):
    n = 1 << (c + 4)
    plan = engine.msm_plan(n, bits, BUCKETS)
    assert plan["c"] == c and cases.straddling_windows(c, plan["windows"])
    order = CURVE_PARAMS[cv]["n"]
    x, y = walk_on_device(engine, cv, n)
    for r, (ks, _) in enumerate(cases.one_hot_batches(c, n, bits)):
        got = run(engine, cv, engine.to_device(cases.limbs_of(ks)), x, y, bits, others=(LANES,))
        assert got == ec_mul(cv, walk_dot(ks, bits, order), G(cv)), (c, bits, r)


# ---- 3. every layout of a bucket over the slices
@pytest.mark.parametrize("n,bits", cases.LAYOUT_SHAPES)
@pytest.mark.parametrize("cv", CURVES)
def test_bucket_boundaries_at_the_slice_edges(engine, cv, n, bits):
    plan = engine.msm_plan(n, bits, BUCKETS)
    assert (plan["c"], plan["windows"], plan["L"]) == {(256, 4): (4, 1, 4), (257, 8): (4, 2, 8), (4099, 8): (8, 1, 32)}[(n, bits)]
    order = CURVE_PARAMS[cv]["n"]
    x, y = walk_on_device(engine, cv, n)
    reached = set()
    for index in range(cases.LAYOUT_BATCHES):
        ks, counts = cases.layout_batch(n, bits, index)
        reached |= cases.layout_classes_of(n, bits, counts)
        kl = np.zeros((n, 4), dtype=np.uint64); kl[:, 0] = ks
        got = run(engine, cv, engine.to_device(kl), x, y, bits, others=(LANES,) if index < cases.LAYOUT_LANES_BATCHES else ())
        assert got == ec_mul(cv, walk_dot(ks, bits, order), G(cv)), (index, counts)
    assert reached == cases.all_layout_classes()


# ---- 4. LANES across a product chunk
def workspace_size(eng):
    ptr, size = C.c_void_p(), C.c_size_t()
    eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
    return int(size.value)


def test_lanes_across_the_product_chunk():
    from ecsimd_amd import Engine
    cv, n, bits = P256, cases.CHUNK_N, cases.CHUNK_BITS
    eng = Engine(0)                                                       # a context of its own: its workspace is what these two calls made it, and goes with it
    try:
        k = cases.chunk_scalars()
        assert k[:, 1:].any(axis=1).all()                                # the upper limbs are there to be ignored
        want = ec_mul(cv, cases.chunk_dot(k, CURVE_PARAMS[cv]["n"]), G(cv))
        kd = eng.to_device(k)
        x, y = walk_on_device(eng, cv, n)
        plans = {alg: eng.msm_plan(n, bits, alg) for alg in (LANES, BUCKETS)}
        assert plans[LANES]["launches"] == 4 + 5 * 2 + model.tree_passes(-(-n // model.TREE_FAN))          # two chunks of the product
        seen = {}
        for alg in (LANES, BUCKETS, BUCKETS):
            seen.setdefault(alg, []).append(call(eng, cv, kd, x, y, bits, alg))
            assert workspace_size(eng) >= plans[alg]["workspace_bytes"] == model.plan(n, bits, alg)["workspace_bytes"], alg
        assert seen[BUCKETS][0] == seen[BUCKETS][1] == seen[LANES][0]
        assert point_of(seen[LANES][0]) == want
    finally:
        eng.close()


# ---- 5. operands nobody has passed yet
def run_point_sum(engine, cv, pts, invalid=0):
    import torch
    x, y = (engine.to_device(cases.limbs_of([p[j] for p in pts])) for j in (0, 1))
    seen = []
    for _ in range(2):
        rx, ry, fin, bad = engine.point_sum(cv, x, y, want_invalid=True)
        torch.cuda.synchronize()
        assert int(bad.cpu()[0]) == invalid
        seen.append((engine.to_numpy(rx).tobytes(), engine.to_numpy(ry).tobytes(), bytes(fin.cpu().numpy())))
    assert seen[0] == seen[1]
    return point_of(seen[0])


def test_the_two_points_of_p256_with_x_zero(engine):
    cv = P256
    p, order = CURVE_PARAMS[cv]["p"], CURVE_PARAMS[cv]["n"]
    yb = cases.sqrt_b(cv)
    Q, Qn = (0, yb), (0, p - yb)
    assert yb and ec_add(cv, Q, Qn) is None and ec_mul(cv, order, Q) is None
    rng = random.Random(0xb)
    rest = list(walk(cv)[:19])
    ks = [rng.getrandbits(256) for _ in range(21)]
    for pts in (rest[:7] + [Q] + rest[7:] + [Q], rest[:7] + [Qn] + rest[7:] + [Q], [Q] + rest + [Qn]):   # ordinary terms
        assert run_ints(engine, cv, ks, pts) == term_by_term(cv, ks, pts)
    for k in (1, 2, order - 1, rng.getrandbits(256)):
        assert run_ints(engine, cv, [k], [Q]) == ec_mul(cv, k % order, Q), k
        assert run_ints(engine, cv, [k, k], [Q, Qn]) is None, k                                         # equal scalars: the sum cancels
        assert run_ints(engine, cv, [k, 5, k], [Q, rest[3], Qn]) == ec_mul(cv, 5, rest[3]), k
        assert run_ints(engine, cv, [k, k], [Q, Q]) == ec_mul(cv, 2 * k % order, Q), k
    assert run_point_sum(engine, cv, [Q]) == Q and run_point_sum(engine, cv, [Qn]) == Qn
    assert run_point_sum(engine, cv, [Q, Qn]) is None
    assert run_point_sum(engine, cv, [Q, Q]) == ec_add(cv, Q, Q)                                        # the tangent at x = 0
    assert run_point_sum(engine, cv, [Q] * 17 + [Qn] * 16) == Q
    want = None
    for P in rest + [Q]: want = ec_add(cv, want, P)
    assert run_point_sum(engine, cv, rest[:5] + [Q] + rest[5:]) == want
    assert run_point_sum(engine, cv, rest + [Q, Qn, Q]) == want


def test_x_zero_is_no_point_of_secp256k1(engine):
    cv = SECP256K1
    p = CURVE_PARAMS[cv]["p"]
    assert cases.sqrt_b(cv) is None and pow(7, (p - 1) // 2, p) == p - 1
    rng = random.Random(7)
    rest = list(walk(cv)[:19])
    ks = [rng.getrandbits(256) for _ in range(23)]
    bad = [(0, 1), (0, pow(7, (p + 1) // 4, p)), (0, p - 1), (0, rng.randrange(1, p))]                  # (0, y), y != 0: never on the curve
    pts = rest[:4] + bad[:2] + rest[4:] + bad[2:]
    want = term_by_term(cv, ks[:4] + ks[6:21], rest)
    assert run_ints(engine, cv, ks, pts, invalid=4) == want
    clean = None
    for P in rest: clean = ec_add(cv, clean, P)
    assert run_point_sum(engine, cv, pts, invalid=4) == clean


@pytest.mark.parametrize("cv", CURVES)
def test_scalars_around_the_group_order(engine, cv):
    order = CURVE_PARAMS[cv]["n"]
    rng = random.Random(0x0de4 + cv)
    edge = cases.order_edge_scalars(cv)
    n = 70
    pts = walk(cv)[:n]
    ks = [rng.getrandbits(256) for _ in range(n)]
    for j, k in enumerate(edge): ks[3 + 13 * j] = k
    ks[n - 1] = order
    want = ec_mul(cv, sum(k * (i + 1) for i, k in enumerate(ks)) % order, G(cv))
    assert run_ints(engine, cv, ks, pts) == want
    for k in edge:                                                        # every lane the same: LANES' product is infinity in every lane for k = order
        assert run_ints(engine, cv, [k] * n, pts) == ec_mul(cv, k * (n * (n + 1) // 2) % order, G(cv)), hex(k)
        assert run_ints(engine, cv, [k], pts[:1]) == ec_mul(cv, k % order, G(cv)), hex(k)
    assert run_ints(engine, cv, [order] * n, pts) is None
    assert run_ints(engine, cv, [order] * 16 + [3] + [order] * 16, pts[:33]) == ec_mul(cv, 3 * 17, G(cv))   # the tree skips sixteen infinities, then meets a point


def test_a_ref_square_compat_context_gives_the_plain_contexts_bytes(engine):
    import torch
    from ecsimd_amd import Engine
    n = 257
    eng = Engine(0)
    try:
        eng.set_ref_square_compat(True)
        for cv in CURVES:
            rng = random.Random(64 + cv)
            ks = [rng.getrandbits(256) for _ in range(n)]
            pts = walk(cv)[:n]
            want = ec_mul(cv, walk_dot(ks, 256, CURVE_PARAMS[cv]["n"]), G(cv))
            arrs = [cases.limbs_of(v) for v in (ks, [p[0] for p in pts], [p[1] for p in pts])]
            out = {}
            for name, e in (("plain", engine), ("compat", eng)):
                k, x, y = (e.to_device(a) for a in arrs)
                out[name] = [call(e, cv, k, x, y, 256, alg) for alg in (BUCKETS, BUCKETS, LANES, AUTO)]
                rx, ry, fin, bad = e.point_sum(cv, x, y, want_invalid=True)
                torch.cuda.synchronize()
                assert int(bad.cpu()[0]) == 0
                out[name].append((e.to_numpy(rx).tobytes(), e.to_numpy(ry).tobytes(), bytes(fin.cpu().numpy())))
            assert out["compat"] == out["plain"]
            assert all(point_of(t) == want for t in out["plain"][:4])
            assert point_of(out["plain"][4]) == ec_mul(cv, n * (n + 1) // 2, G(cv))
    finally:
        eng.close()
