"""GPU suite: the bucket method on the twisted Edwards curve (include/ecsimd_ed25519_batch.h, Engine.ed25519_msm).

Terms are P_i = [t_i]B + T_i with t_i known and T_i one of the eight torsion points, so the expected sum is one base multiplication and one small torsion
multiple on the host (tools/ed25519_model.py): [sum k_i t_i mod L]B + sum [k_i mod 8]T_i -- the exact INTEGER combination, which the device has to match with
scalars at and above L.  Every case also goes through tools/ed25519_batch_model.py's term-by-term sum at the small sizes.  The two large cases (window widths
12 and 16) take their points from the device's own constant-time comb (ECSIMD_ED25519_RAW_BASE_MULT)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as ed             # noqa: E402
import ed25519_batch_model as model    # noqa: E402

pytestmark = pytest.mark.gpu
L = ed.L
IDENTITY_ENC = ed.SMALL_ORDER[0]
RAW_BASE_MULT = 12
SIZES = (1, 2, 17, 300)
BITS = (1, 4, 128, 253, 256)


def le32(v):
    return int(v).to_bytes(32, "little")


def dev_rows(engine, rows, width=32):
    import torch
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy() if rows else np.zeros((0, width), dtype=np.uint8)
    return torch.from_numpy(a).to(engine.tdev)


@functools.lru_cache(maxsize=None)
def torsion():
    return tuple(t for _, t, _ in ed.torsion())


@functools.lru_cache(maxsize=None)
def term(t, tors):
    """The encoding of [t]B + T_tors."""
    return ed.encode(ed.pt_add(ed.base_point_mul(t), torsion()[tors]))


@functools.lru_cache(maxsize=None)
def terms(n, with_torsion):
    """n (t, torsion index) pairs, fixed; without torsion every index is 0 (the identity)."""
    rng = np.random.default_rng(77 + n)
    return tuple((int.from_bytes(rng.bytes(32), "little") % L, (i % 8) if with_torsion else 0) for i in range(n))


def expected(ks, ts, bits=256):
    """(encoding, finite) of sum (k_i mod 2^bits) ([t_i]B + T_i)."""
    mask = (1 << bits) - 1
    acc = ed.base_point_mul(sum((k & mask) * t for k, (t, _) in zip(ks, ts)) % L)
    for j, T in enumerate(torsion()):
        acc = ed.pt_add(acc, ed.pt_mul(sum((k & mask) for k, (_, tj) in zip(ks, ts) if tj == j) % 8, T))
    return ed.encode(acc), int(not ed.pt_eq(acc, ed.IDENTITY))


def run(engine, ks, encs, bits=256, alg=0):
    out, finite, invalid = engine.ed25519_msm(dev_rows(engine, [le32(k) for k in ks]), dev_rows(engine, list(encs)), bits=bits, alg=alg, want_invalid=True)
    return bytes(out.cpu().numpy()), int(finite.cpu()[0]), int(invalid.cpu()[0])


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(n)]


# ---------------------------------------------------------------- 1. sizes and widths against the integer combination
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_bit_lengths_against_the_integer_combination(engine, n):
    ts = terms(n, True)
    encs = [term(t, j) for t, j in ts]
    ks = scalars(n, 5 * n)
    ks[0] = (1 << 256) - 1
    if n > 1:
        ks[1] = L + 8 * 0 + 5                                             # at and above L: the scalar is an integer, not a residue
    for bits in BITS:
        plan = engine.ed25519_msm_plan(n, bits)
        got = run(engine, ks, encs, bits, alg=bits % 2)                   # (0 and ECSIMD_MSM_ALG_BUCKETS are the same route)
        enc, fin = expected(ks, ts, bits)
        assert got == (enc, fin, 0), (n, bits, plan)
        if n <= 17:
            assert (enc, fin, 0) == model.msm_encoded(ks, encs, bits), (n, bits)      # the two host statements agree
    assert run(engine, ks, encs, 256) == run(engine, ks, encs, 256)


def test_the_empty_sum_is_the_identity(engine):
    assert run(engine, [], []) == (IDENTITY_ENC, 0, 0)


# ---------------------------------------------------------------- 2. scalars
def test_scalar_patterns_at_300_terms(engine):
    n = 300
    ts = terms(n, True)
    encs = [term(t, j) for t, j in ts]
    plan = engine.ed25519_msm_plan(n, 256)
    assert plan["L"] == 8 and n > plan["L"]                               # equal scalars: one run of 300 entries per window, split across 38 slices
    for name, ks in (("all zero", [0] * n), ("all equal", [0x1234567890ABCDEF1122334455667788 << 100 | 0xF00D] * n), ("all equal and small", [3] * n),
                     ("all ones", [(1 << 256) - 1] * n), ("L and its neighbours", [L - 1, L, L + 1] * 100), ("one nonzero", [0] * 299 + [L + 7])):
        for bits in (253, 256):
            assert run(engine, ks, encs, bits) == expected(ks, ts, bits) + (0,), (name, bits)
    assert run(engine, [0] * n, encs) == (IDENTITY_ENC, 0, 0)
    for bits in BITS:
        ks = [(1 << bits) - 1] * n
        assert run(engine, ks, encs, bits) == expected(ks, ts, bits) + (0,), bits
        assert run(engine, [(1 << 256) - 1] * n, encs, bits) == expected(ks, ts, bits) + (0,), bits      # only the low `bits` bits are read


# ---------------------------------------------------------------- 3. points
def test_point_patterns_the_complete_addition_has_no_exception(engine):
    n = 300
    ks = scalars(n, 9)
    # the identity as every term; the identity among others
    assert run(engine, ks, [IDENTITY_ENC] * n) == (IDENTITY_ENC, 0, 0)
    ts = list(terms(n, False))
    encs = [term(t, 0) for t, _ in ts]
    mixed_encs = list(encs); mixed_ts = list(ts)
    for i in range(0, n, 7):
        mixed_encs[i] = IDENTITY_ENC; mixed_ts[i] = (0, 0)
    assert run(engine, ks, mixed_encs) == expected(ks, mixed_ts) + (0,)
    # P beside -P under the same scalar: every bucket that gets one gets the other; then with different scalars
    t = ts[3][0]
    pair = [term(t, 0), term(L - t, 0)]
    assert run(engine, [ks[0], ks[0]], pair) == (IDENTITY_ENC, 0, 0)
    assert run(engine, [ks[0]] * n, pair * (n // 2)) == (IDENTITY_ENC, 0, 0)
    assert run(engine, ks[:2], pair) == expected(ks[:2], [(t, 0), (L - t, 0)]) + (0,)
    # the same P 300 times: equal scalars (P + P in every bucket, in every slot, up the tree) and different ones
    same = [term(t, 0)] * n
    assert run(engine, [ks[5]] * n, same) == expected([ks[5]] * n, [(t, 0)] * n) + (0,)
    assert run(engine, ks, same) == expected(ks, [(t, 0)] * n) + (0,)


def test_each_torsion_component_with_scalars_at_and_above_L(engine):
    for j in range(8):
        ts = [(1000 + i, j) for i in range(17)]
        encs = [term(t, j) for t, _ in ts]
        ks = [L + i for i in range(9)] + [8 * L + 3, (1 << 256) - 1 - j, L - 1, 2 * L, 1, 7, 8, (1 << 255) + 4]
        want = expected(ks, ts)
        assert run(engine, ks, encs) == want + (0,), j
        assert want[:2] == model.msm_encoded(ks, encs)[:2]
    # the torsion points themselves, all eight: sum k_j T_j
    encs = [term(0, j) for j in range(8)]
    assert tuple(encs) == ed.SMALL_ORDER
    ks = [L + 1 + j for j in range(8)]
    assert run(engine, ks, encs) == expected(ks, [(0, j) for j in range(8)]) + (0,)
    assert run(engine, [8 * (L + j) for j in range(8)], encs) == (IDENTITY_ENC, 0, 0)


def test_encodings_that_do_not_decode_are_counted_and_contribute_nothing(engine):
    n = 300
    ts = list(terms(n, True))
    encs = [term(t, j) for t, j in ts]
    ks = scalars(n, 31)
    refused = ed.refused_encodings()
    where = list(range(0, n, 11))[:len(refused)]
    for i, e in zip(where, refused):
        encs[i] = e; ts[i] = (0, 0)
    assert len(where) == len(refused) == 26
    assert run(engine, ks, encs) == expected(ks, ts) + (26,)
    assert run(engine, ks[:3], refused[:3]) == (IDENTITY_ENC, 0, 3)


# ---------------------------------------------------------------- 4. the wide windows
@pytest.mark.parametrize("log_n,c", ((16, 12), (20, 16)))
def test_wide_windows_against_one_host_base_multiplication(engine, log_n, c):
    import torch
    n = 1 << log_n
    plan = engine.ed25519_msm_plan(n, 256)
    assert plan["c"] == c and plan["windows"] * c >= 256
    rng = np.random.default_rng(log_n)
    tb, kb = rng.bytes(32 * n), rng.bytes(32 * n)
    t_rows = torch.from_numpy(np.frombuffer(tb, dtype=np.uint8).reshape(n, 32).copy()).to(engine.tdev)
    k_rows = torch.from_numpy(np.frombuffer(kb, dtype=np.uint8).reshape(n, 32).copy()).to(engine.tdev)
    pts = engine.ed25519_raw(RAW_BASE_MULT, t_rows)                       # P_i = [t_i mod L]B, by the device's comb
    out, finite, invalid = engine.ed25519_msm(k_rows, pts, bits=256, want_invalid=True)
    total = 0
    for i in range(n):
        total += int.from_bytes(kb[32 * i:32 * i + 32], "little") * (int.from_bytes(tb[32 * i:32 * i + 32], "little") % L)
    assert bytes(out.cpu().numpy()) == ed.base_mult(total % L)
    assert int(finite.cpu()[0]) == 1 and int(invalid.cpu()[0]) == 0


# ---------------------------------------------------------------- 5. arguments and capture
def test_bad_arguments_are_refused_and_the_outputs_untouched(engine):
    import ctypes as C
    import torch
    n = 17
    ts = terms(n, False)
    k = dev_rows(engine, [le32(x) for x in scalars(n, 1)]); pts = dev_rows(engine, [term(t, 0) for t, _ in ts])
    out = torch.full((64,), 0xAA, dtype=torch.uint8, device=engine.tdev)
    inv = torch.zeros((2,), dtype=torch.int32, device=engine.tdev)
    torch.cuda.synchronize()
    engine._bind_stream()
    lib = engine.lib
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(kp=ptr(k), pp=ptr(pts), op=ptr(out), fp=ptr(out, 40), ip=ptr(inv), n=n, bits=256, flags=0):
        rc = lib.ecsimd_ed25519_msm(engine.ctx, kp, pp, op, fp, ip, C.c_size_t(n), C.c_int(bits), C.c_int(flags))
        return rc, lib.ecsimd_hip_last_error(engine.ctx).decode()
    null = C.c_void_p(0)
    cases = {"LANES": call(flags=2), "flag 4": call(flags=4), "flag -1": call(flags=-1), "bits 0": call(bits=0), "bits 257": call(bits=257),
             "k null": call(kp=null), "pts null": call(pp=null), "out null": call(op=null), "finite null": call(fp=null), "invalid misaligned": call(ip=ptr(inv, 2)),
             "out inside k": call(op=ptr(k, 32 * n - 1)), "finite inside pts": call(fp=ptr(pts, 5)), "finite inside out": call(fp=ptr(out, 31)),
             "n too large": call(n=(1 << 24) + 1)}
    for name, (rc, said) in cases.items():
        assert rc == -1 and said.startswith("bad argument: ") and len(said) > 20, (name, rc, said)
    assert "bucket" in cases["LANES"][1] and "overlap" in cases["out inside k"][1] and "MAX_N" in cases["n too large"][1]
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == b"\xaa" * 64
    assert call(ip=null)[0] == 0
    torch.cuda.synchronize()
    got = bytes(out.cpu().numpy())
    ks = [int.from_bytes(bytes(r), "little") for r in k.cpu().numpy()]
    assert (got[:32], got[40]) == expected(ks, ts) and got[32:40] + got[41:] == b"\xaa" * 31


def test_a_captured_sum_replays_and_a_cold_capture_is_refused(engine):
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    n = 300
    ts = terms(n, True)
    ks = scalars(n, 3)
    k = dev_rows(engine, [le32(x) for x in ks]); pts = dev_rows(engine, [term(t, j) for t, j in ts])
    torch.cuda.synchronize()
    eng = Engine(0)
    try:
        said = []
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())

        def capture(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    res = fn()
            torch.cuda.synchronize()
            return g, res

        def cold():
            try:
                eng.ed25519_msm(k, pts)
            except EcsimdHipError as exc:
                said.append(str(exc))
        g, _ = capture(cold)
        assert len(said) == 1 and "capture" in said[0] and "(-1)" in said[0]
        del g
        eng.ed25519_msm(k, pts)                                           # the warm-up
        torch.cuda.synchronize()
        g, (out, finite) = capture(lambda: eng.ed25519_msm(k, pts))
        g.replay(); torch.cuda.synchronize()
        assert (bytes(out.cpu().numpy()), int(finite.cpu()[0])) == expected(ks, ts)
        k[7] = torch.zeros(32, dtype=torch.uint8, device=eng.tdev)
        torch.cuda.synchronize()
        g.replay(); torch.cuda.synchronize()
        assert (bytes(out.cpu().numpy()), int(finite.cpu()[0])) == expected(ks[:7] + [0] + ks[8:], ts)
        del g
    finally:
        eng.close()
