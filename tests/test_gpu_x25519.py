"""GPU suite for X25519 (include/ecsimd_x25519.h).  Every expected value comes from tools/x25519_model.py (plain Python integers; its Edwards route from
tools/ed25519_model.py) or from tests/golden/x25519_vectors.json (RFC 7748 5.2 and 6.1 and records minted from libcrypto).  Layer by layer through
ecsimd_x25519_raw, then the four calls: the fixture bit for bit, RFC 7748's 1000-fold iteration, unaligned arrays, the small-order and non-canonical u, both
routes to a public key against each other, Ed25519 keys with a small-order component, the chunk boundary, graph capture on a fresh context, and the untouched workspace."""
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
import ed25519_model as ed      # noqa: E402
import x25519_model as model    # noqa: E402

pytestmark = pytest.mark.gpu
P, L = model.P, model.L
le32 = model.le32
OP = dict(FE_MUL_SMALL=0, LADDER=1, ED_TO_MONT=2)
EDGE = (0, 1, 2, 19, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1, 2**256 - 38, 2**256 - 39)       # tests/test_gpu_ed25519.py's
LADDER_SCALARS = (0, 1, 2, 3, 7, 8, L - 1, L, L + 1, 2 * L, 2**252, 2**254, 2**255 - 1)
ZERO32 = bytes(32)


def dev_rows(engine, rows, width=32, offset=None):
    """A list of byte strings of `width` bytes -> an (n, width) uint8 device tensor; with offset a view at that byte offset inside a larger allocation."""
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    t = torch.from_numpy(a).to(engine.tdev)
    if offset is None:
        return t
    buf = torch.zeros(width * len(rows) + 8, dtype=torch.uint8, device=engine.tdev)
    view = buf[offset:offset + width * len(rows)].view(len(rows), width)
    view.copy_(t)
    assert view.data_ptr() % 4 == offset % 4
    return view


def host_rows(t):
    return [bytes(r) for r in t.cpu().numpy()]


def raw(engine, op, *columns):
    n = len(columns[0])
    rec = [b"".join(c[i] for c in columns) for i in range(n)]
    out = host_rows(engine.x25519_raw(OP[op], dev_rows(engine, rec, 32 * len(columns))))
    return [[o[k:k + 32] for k in range(0, len(o), 32)] for o in out]


@functools.lru_cache(maxsize=None)
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "x25519_vectors.json")))


@functools.lru_cache(maxsize=None)
def model_x25519(k, u):
    return model.x25519(k, u)


@functools.lru_cache(maxsize=None)
def model_base(k):
    return model.x25519_base(k)


@functools.lru_cache(maxsize=None)
def curve_and_twist_points():
    """six u on the curve and six on its twist"""
    rng = random.Random(486662)
    on, off = [], []
    while len(on) < 6 or len(off) < 6:
        u = rng.randrange(2, P)
        (on if model.on_curve(u) else off).append(u)
    return tuple(on[:6]), tuple(off[:6])


@functools.lru_cache(maxsize=None)
def tile_inputs():
    """4096 distinct (scalar, u) pairs, made once"""
    rng = random.Random(4096)
    return tuple(rng.randbytes(32) for _ in range(4096)), tuple(rng.randbytes(32) for _ in range(4096))


# ---- the layers
def test_raw_fe_mul_small_against_integers(engine):
    rng = random.Random(121665)
    values = list(EDGE) + [rng.getrandbits(256) for _ in range(300 - len(EDGE))]
    out = raw(engine, "FE_MUL_SMALL", [le32(v) for v in values])
    assert [int.from_bytes(o[0], "little") for o in out] == [v * 121665 % P for v in values]


def test_raw_ladder_on_every_scalar_and_every_kind_of_u(engine):
    on, off = curve_and_twist_points()
    us = [9] + list(on) + list(off) + [0, 1, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1]
    pairs = [(k, u) for k in LADDER_SCALARS for u in us]
    out = raw(engine, "LADDER", [le32(k) for k, _ in pairs], [le32(u) for _, u in pairs])
    got = [int.from_bytes(o[0], "little") for o in out]
    assert got == [model.ladder(k, u) for k, u in pairs]
    by = dict(zip(pairs, got))
    for k in LADDER_SCALARS:
        assert by[(k, 9)] == model.edwards_base(k), k                                                # the other curve model agrees on the base point
    assert by[(0, 9)] == 0 and by[(L, 9)] == 0 and by[(1, 9)] == 9 and by[(L + 1, 9)] == 9            # infinity is 0
    assert by[(2**255 - 1, 2**256 - 1)] == model.ladder(2**255 - 1, (2**256 - 1) % P)                 # any representative of u


def test_raw_ed_to_mont(engine):
    rng = random.Random(25519)
    good = [ed.base_mult(rng.randrange(1, L)) for _ in range(24)] + [ed.encode(ed.B)]
    good += [ed.encode(ed.pt_neg(ed.decode(e))) for e in good[:8]]
    refused = [le32(P + i) for i in range(19)] + [le32(1 | (1 << 255)), le32((P - 1) | (1 << 255)), le32(2), le32(2 | (1 << 255)), le32(7), bytes([0xff]) * 32]
    encs = good + refused + list(ed.SMALL_ORDER)
    out = raw(engine, "ED_TO_MONT", encs)
    for e, o in zip(encs, out):
        u, ok = model.from_ed25519_pk(e)
        assert o == [u, le32(ok)], e.hex()
    assert all(o[1] == le32(1) for o in out[:len(good)]) and all(o == [ZERO32, le32(0)] for o in out[len(good):])
    assert out[24][0] == model.NINE and [o[0] for o in out[25:33]] == [o[0] for o in out[:8]]       # B -> 9; the sign of x is dropped


# ---- x25519
def run_x25519(engine, ks, us, offset=None, want_ok=True):
    res = engine.x25519(dev_rows(engine, ks, 32, offset), dev_rows(engine, us, 32, offset), want_ok=want_ok)
    return (host_rows(res[0]), res[1].cpu().tolist()) if want_ok else host_rows(res)


def test_the_fixture_bit_for_bit(engine):
    cases = fixture()["cases"]
    ks, us = [bytes.fromhex(c["scalar"]) for c in cases], [bytes.fromhex(c["u"]) for c in cases]
    out, ok = run_x25519(engine, ks, us)
    assert [o.hex() for o in out] == [c["out"] for c in cases]
    assert ok == [c["ok"] for c in cases] and 0 in ok and 1 in ok
    assert run_x25519(engine, ks, us, want_ok=False) == out                                           # ok = NULL is accepted
    assert out[0].hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"         # RFC 7748 5.2


def test_rfc_7748_iterated_a_thousand_times_on_65_lanes(engine):
    import torch
    want = fixture()["iterated"]
    k = dev_rows(engine, [model.NINE] * 65)
    u = k.clone()
    for i in range(1, 1001):
        k, u = engine.x25519(k, u), k
        if i == 1:
            assert host_rows(k) == [bytes.fromhex(want["1"])] * 65
    torch.cuda.synchronize()
    assert host_rows(k) == [bytes.fromhex(want["1000"])] * 65


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_batch_sizes_with_every_array_at_byte_offset_one(engine, n):
    import torch
    ks, us = tile_inputs()
    ks, us = list(ks[:n]), list(us[:n])
    kt, ut = dev_rows(engine, ks, 32, 1), dev_rows(engine, us, 32, 1)
    ob = torch.zeros(32 * n + 8, dtype=torch.uint8, device=engine.tdev)
    out = ob[1:1 + 32 * n].view(n, 32)
    ok = torch.zeros(n + 8, dtype=torch.uint8, device=engine.tdev)[1:1 + n]
    engine._bind_stream()
    engine._check(engine.lib.ecsimd_x25519(engine.ctx, C.c_void_p(kt.data_ptr()), C.c_void_p(ut.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ok.data_ptr()),
                                           C.c_size_t(n)), "x25519")
    assert host_rows(out) == [model_x25519(k, u) for k, u in zip(ks, us)]
    assert ok.cpu().tolist() == [1] * n and ob[0].item() == 0 and not ob[1 + 32 * n:].any().item()    # nothing outside the view was written
    assert host_rows(engine.x25519_base(kt)) == [model_base(k) for k in ks]                           # the comb route, the scalars unaligned
    sc = torch.zeros(32 * n + 8, dtype=torch.uint8, device=engine.tdev)[1:1 + 32 * n].view(n, 32)
    engine._check(engine.lib.ecsimd_x25519_from_ed25519_seed(engine.ctx, C.c_void_p(kt.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_size_t(n)), "from_seed")
    assert host_rows(sc)[:64] == [model.from_ed25519_seed(k) for k in ks[:64]]


def test_small_order_and_non_canonical_u(engine):
    rng = random.Random(61)
    small = [e for u in model.SMALL_ORDER_U for e in (le32(u), le32(u | (1 << 255)))]
    assert len(small) == 14
    other = [le32(u | top) for u in [P - 3, P - 2, 2**255 - 1] + [P + i for i in range(2, 19)] for top in (0, 1 << 255)]
    us = small + other
    ks = [rng.randbytes(32) for _ in us]
    out, ok = run_x25519(engine, ks, us)
    assert out[:14] == [ZERO32] * 14 and ok[:14] == [0] * 14
    assert ok[14:] == [1] * len(other) and ZERO32 not in out[14:]
    assert out == [model_x25519(k, u) for k, u in zip(ks, us)]
    canon = [le32((int.from_bytes(u, "little") & (2**255 - 1)) % P) for u in us]                     # bit 255 ignored, the residue counts
    assert run_x25519(engine, ks, canon)[0] == out


# ---- x25519_base
def test_the_comb_route_is_the_ladder_on_nine_and_the_model(engine):
    rng = random.Random(9)
    d = fixture()["dh"]
    ks = [bytes(32), bytes([0xff]) * 32, bytes.fromhex(d["a"]), bytes.fromhex(d["b"])] + [rng.randbytes(32) for _ in range(126)]
    got = host_rows(engine.x25519_base(dev_rows(engine, ks)))
    assert got == run_x25519(engine, ks, [model.NINE] * len(ks), want_ok=False)
    assert got == [model_base(k) for k in ks]
    assert got[2].hex() == d["a_public"] and got[3].hex() == d["b_public"]


def test_dh_symmetry_on_300_pairs(engine):
    rng = random.Random(300)
    a, b = [rng.randbytes(32) for _ in range(300)], [rng.randbytes(32) for _ in range(300)]
    ta, tb = dev_rows(engine, a), dev_rows(engine, b)
    pa, pb = engine.x25519_base(ta), engine.x25519_base(tb)
    sa, oka = engine.x25519(ta, pb, want_ok=True)
    sb, okb = engine.x25519(tb, pa, want_ok=True)
    assert host_rows(sa) == host_rows(sb) and oka.cpu().tolist() == okb.cpu().tolist() == [1] * 300
    assert host_rows(sa)[:16] == [model_x25519(x, model_base(y)) for x, y in zip(a[:16], b[:16])]
    d = fixture()["dh"]
    one = engine.x25519(dev_rows(engine, [bytes.fromhex(d["a"])]), dev_rows(engine, [bytes.fromhex(d["b_public"])]))
    assert host_rows(one)[0].hex() == d["shared"]


# ---- the conversions
def test_both_conversions_and_the_seed_pk_property(engine):
    rng = random.Random(32)
    seeds = [bytes(32), bytes([0xff]) * 32] + [rng.randbytes(32) for _ in range(98)]
    st = dev_rows(engine, seeds)
    sc = engine.x25519_from_ed25519_seed(st)
    assert host_rows(sc) == [model.from_ed25519_seed(s) for s in seeds]
    pk = engine.ed25519_pubkey(st)
    u, ok = engine.x25519_from_ed25519_pk(pk)
    assert ok.cpu().tolist() == [1] * len(seeds)
    assert host_rows(u) == host_rows(engine.x25519_base(sc))                                          # end to end on the device
    assert host_rows(u)[:20] == [model.from_ed25519_pk(ed.pubkey(s))[0] for s in seeds[:20]]
    bad = list(ed.SMALL_ORDER) + [le32(P + 1), le32(2), le32(1 | (1 << 255))]
    keys = bad + host_rows(pk)[:5]
    u, ok = engine.x25519_from_ed25519_pk(dev_rows(engine, keys, 32, 1))
    assert ok.cpu().tolist() == [0] * len(bad) + [1] * 5
    assert host_rows(u) == [model.from_ed25519_pk(e)[0] for e in keys] and host_rows(u)[:len(bad)] == [ZERO32] * len(bad)


def test_ed25519_keys_with_a_small_order_component(engine):
    """A + T for 8 prime-order A = [a]B and the 7 non-zero torsion points T.  Every expected value is made on the Edwards curve and mapped by
    u = (1 + y) / (1 - y): the conversion checks no subgroup, the raw ladder sees the torsion, and the clamp (a multiple of 8) removes it."""
    rng = random.Random(56)
    tors = ed.torsion()
    keys = model.mixed_keys([rng.randrange(1, L) for _ in range(8)])
    encs = [ed.encode(m) for _, _, _, m in keys]
    u_mixed = [model.u_of_encoding(e) for e in encs]
    u_pure = [model.u_of_encoding(ed.encode(pt)) for _, _, pt, _ in keys]
    assert len(keys) == 56 and not set(encs) & set(ed.SMALL_ORDER) and all(x != y for x, y in zip(u_mixed, u_pure))
    u, ok = engine.x25519_from_ed25519_pk(dev_rows(engine, encs))
    assert ok.cpu().tolist() == [1] * 56
    assert host_rows(u) == [le32(x) for x in u_mixed] == [model.from_ed25519_pk(e)[0] for e in encs]
    # x25519 under 16 scalars: the same shared secret as the prime-order key's, [clamp(k) a]B on the Edwards curve
    ks = [rng.randbytes(32) for _ in range(16)]
    assert all(any(k[0] >> bit & 1 for k in ks) for bit in range(3))                                # the clamp has each of the three bits to clear
    lanes = [(k, i) for i in range(56) for k in ks]
    shared = {(k, a): le32(model.edwards_base(model.clamp(int.from_bytes(k, "little")) * a)) for k in ks for a in {key[0] for key in keys}}
    want = [shared[(k, keys[i][0])] for k, i in lanes]
    got_mixed, ok_mixed = run_x25519(engine, [k for k, _ in lanes], [le32(u_mixed[i]) for _, i in lanes])
    got_pure, ok_pure = run_x25519(engine, [k for k, _ in lanes], [le32(u_pure[i]) for _, i in lanes])
    assert got_mixed == want and got_pure == want and ok_mixed == ok_pure == [1] * len(lanes)
    assert got_mixed[:32] == [model_x25519(k, le32(u_mixed[i])) for k, i in lanes[:32]]               # ... and the ladder model's
    # the ladder itself, unclamped: k = 1 gives u back; k = L + 1 (6 modulo 8) leaves A + [6]T, which is A only where T has order 2
    one = raw(engine, "LADDER", [le32(1)] * 112, [le32(x) for x in u_mixed + u_pure])
    assert [int.from_bytes(o[0], "little") for o in one] == u_mixed + u_pure
    more = [int.from_bytes(o[0], "little") for o in raw(engine, "LADDER", [le32(L + 1)] * 112, [le32(x) for x in u_mixed + u_pure])]
    assert more[56:] == u_pure
    assert more[:56] == [model.ed_point_to_u(ed.pt_add(pt, ed.pt_mul((L + 1) % 8, tors[j][1]))) for _, j, pt, _ in keys]
    assert [x != y for x, y in zip(more[:56], more[56:])] == [tors[j][2] != 2 for _, j, _, _ in keys]


# ---- the chunk boundary
def test_one_call_across_the_chunk_boundary(engine):
    """A call walks its batch in chunks of 2^20 lanes: 4096 distinct inputs tiled over 2^20 + 65 lanes."""
    import torch
    tile, n = 4096, (1 << 20) + 65
    ks, us = tile_inputs()
    reps = (n + tile - 1) // tile
    kt = dev_rows(engine, list(ks)).repeat(reps, 1)[:n].contiguous()
    ut = dev_rows(engine, list(us)).repeat(reps, 1)[:n].contiguous()
    out, ok = engine.x25519(kt, ut, want_ok=True)
    assert torch.equal(out, out[:tile].repeat(reps, 1)[:n])                                           # compared on the device
    assert bool((ok == 1).all().item())
    rng = random.Random(65)
    lanes = sorted(set(rng.sample(range(n - 65), 191)) | set(range(n - 65, n)))
    assert len(lanes) == 256
    got = host_rows(out[torch.tensor(lanes, device=engine.tdev)])
    assert got == [model_x25519(ks[i % tile], us[i % tile]) for i in lanes]


# ---- graph capture
def test_capture_of_the_four_calls_on_a_fresh_context_without_a_warm_up():
    import torch
    from ecsimd_amd import Engine
    n = 130
    rng = random.Random(4)
    sets = []
    for _ in range(3):
        ks, us, seeds = ([rng.randbytes(32) for _ in range(n)] for _ in range(3))
        us[7] = le32(1); us[64] = le32(P)                                                             # small order: zeros and ok = 0
        pks = [ed.base_mult(rng.randrange(1, L)) for _ in range(n)]
        pks[5] = ed.SMALL_ORDER[4]
        sets.append(dict(k=ks, u=us, seed=seeds, pk=pks))
    eng = Engine(0)
    try:
        bufs = {name: dev_rows(eng, sets[0][name]) for name in ("k", "u", "seed", "pk")}
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):                                                    # nothing has run on this context before
                out = dict(x=eng.x25519(bufs["k"], bufs["u"], want_ok=True), base=eng.x25519_base(bufs["k"]), pk=eng.x25519_from_ed25519_pk(bufs["pk"]),
                           seed=eng.x25519_from_ed25519_seed(bufs["seed"]))
        torch.cuda.synchronize()
        for i in (1, 2):
            for name in bufs:
                bufs[name].copy_(dev_rows(eng, sets[i][name]))
            torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            s = sets[i]
            want = [model_x25519(k, u) for k, u in zip(s["k"], s["u"])]
            assert host_rows(out["x"][0]) == want and out["x"][1].cpu().tolist() == [model.ok_of(w) for w in want], i
            assert want[7] == ZERO32 and want[64] == ZERO32
            assert host_rows(out["base"]) == [model_base(k) for k in s["k"]], i
            conv = [model.from_ed25519_pk(e) for e in s["pk"]]
            assert host_rows(out["pk"][0]) == [c[0] for c in conv] and out["pk"][1].cpu().tolist() == [c[1] for c in conv] and conv[5][1] == 0, i
            assert host_rows(out["seed"]) == [model.from_ed25519_seed(x) for x in s["seed"]], i
        del g
    finally:
        eng.close()


# ---- the workspace
def test_no_call_touches_the_workspace():
    import torch
    from ecsimd_amd import Engine
    eng = Engine(0)
    try:
        n = 300
        rng = random.Random(12)
        seeds = dev_rows(eng, [rng.randbytes(32) for _ in range(n)])
        us = dev_rows(eng, [rng.randbytes(32) for _ in range(n)])
        pk = eng.ed25519_pubkey(seeds); torch.cuda.synchronize()                                      # sizes the workspace
        ptr, size = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(ptr), C.byref(size)), "workspace_info")
        assert ptr.value and size.value >= 32 * n
        fill = np.full(size.value, 0xA5, dtype=np.uint8)
        eng._bind_stream()
        eng._check(eng.lib.ecsimd_hip_memcpy_h2d(eng.ctx, ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(size.value)), "memcpy_h2d")
        eng.x25519(seeds, us, want_ok=True); eng.x25519_base(seeds); eng.x25519_from_ed25519_pk(pk); eng.x25519_from_ed25519_seed(seeds)
        torch.cuda.synchronize()
        p2, s2 = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.ecsimd_hip_workspace_info(eng.ctx, C.byref(p2), C.byref(s2)), "workspace_info")
        assert (p2.value, s2.value) == (ptr.value, size.value)
        back = np.empty(size.value, dtype=np.uint8)
        eng._check(eng.lib.ecsimd_hip_memcpy_d2h(eng.ctx, back.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(size.value)), "memcpy_d2h")
        assert (back == 0xA5).all(), np.flatnonzero(back != 0xA5)[:8]
    finally:
        eng.close()


# ---- arguments
def test_empty_batches_and_refused_arguments(engine):
    import torch
    from ecsimd_amd.engine import EcsimdHipError
    e32 = torch.zeros((0, 32), dtype=torch.uint8, device=engine.tdev)
    out, ok = engine.x25519(e32, e32, want_ok=True)
    assert out.shape == (0, 32) and ok.shape == (0,)
    assert engine.x25519_base(e32).shape == (0, 32) and engine.x25519_from_ed25519_seed(e32).shape == (0, 32)
    u, ok = engine.x25519_from_ed25519_pk(e32)
    assert u.shape == (0, 32) and ok.shape == (0,)
    assert engine.x25519_raw(OP["LADDER"], torch.zeros((0, 64), dtype=torch.uint8, device=engine.tdev)).shape == (0, 32)
    a, b, c = (torch.zeros((2, 32), dtype=torch.uint8, device=engine.tdev) for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())
    lib, ctx, two = engine.lib, engine.ctx, C.c_size_t(2)
    engine._bind_stream()
    for what, call, text in (
            ("x25519 null", lambda: lib.ecsimd_x25519(ctx, p(a), None, p(c), None, two), "is null"),
            ("x25519 out = u", lambda: lib.ecsimd_x25519(ctx, p(a), p(b), p(b), None, two), "must not alias"),
            ("x25519 ok = out", lambda: lib.ecsimd_x25519(ctx, p(a), p(b), p(c), p(c), two), "must not alias"),
            ("base null", lambda: lib.ecsimd_x25519_base(ctx, None, p(c), two), "is null"),
            ("base alias", lambda: lib.ecsimd_x25519_base(ctx, p(a), p(a), two), "must not alias"),
            ("pk null ok", lambda: lib.ecsimd_x25519_from_ed25519_pk(ctx, p(a), p(b), None, two), "is null"),
            ("pk alias", lambda: lib.ecsimd_x25519_from_ed25519_pk(ctx, p(a), p(a), p(c), two), "must not alias"),
            ("seed null", lambda: lib.ecsimd_x25519_from_ed25519_seed(ctx, p(a), None, two), "is null"),
            ("seed alias", lambda: lib.ecsimd_x25519_from_ed25519_seed(ctx, p(a), p(a), two), "must not alias"),
            ("raw null", lambda: lib.ecsimd_x25519_raw(ctx, C.c_int(0), None, p(c), two), "null pointer"),
            ("raw alias", lambda: lib.ecsimd_x25519_raw(ctx, C.c_int(0), p(a), p(a), two), "must not alias"),
            ("raw op", lambda: lib.ecsimd_x25519_raw(ctx, C.c_int(3), p(a), p(c), two), "unknown function")):
        with pytest.raises(EcsimdHipError, match=text):
            engine._check(call(), what)
    with pytest.raises(EcsimdHipError, match="unknown function"):
        engine.x25519_raw(7, a)
    cases = fixture()["cases"][:6]
    ks, us = [bytes.fromhex(c["scalar"]) for c in cases], [bytes.fromhex(c["u"]) for c in cases]
    engine.set_ref_square_compat(True)                                           # accepted: the same bytes
    try:
        assert [o.hex() for o in run_x25519(engine, ks, us)[0]] == [c["out"] for c in cases]
        assert host_rows(engine.x25519_base(dev_rows(engine, ks))) == [model_base(k) for k in ks]
    finally:
        engine.set_ref_square_compat(False)
