"""GPU suite: ECDSA public-key recovery (ecsimd_hip_ecdsa_recover) and signing with the recovery id (ecsimd_hip_ecdsa_sign_recoverable).

Expected values come from three places, none of them the code under test: OpenSSL's libcrypto (k G and d G on the two built-in curves), the host model
on Python integers (tools/ecdsa_recover_model.py, itself checked against the textbook ec_mul by tests/test_ecdsa_recover_cpu.py), and the engine's OTHER
public calls chained (gfp_inverse, mod_mul, gfp_opposite, compute_y, a parity select, double_scalar_mult), which must give the same bits.
"""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add, ec_mul, from_int, to_int, ints_to_arr, arr_to_ints

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ecdsa_recover_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
THREADS = 16
BUILT_IN = ["p256", "secp256k1"]
ALL = BUILT_IN + ["brainpoolP256r1", "sm2", "frp256v1"]


class Spec:
    """One curve: its id, its parameters, the field id of its group order."""
    def __init__(self, name):
        from ecsimd_amd.curves import NAMED, curve_id
        from ecsimd_amd.engine import ORDER_FIELD, register_modulus
        self.name, self.id = name, curve_id(name)
        self.c = CURVE_PARAMS[self.id] if name in BUILT_IN else NAMED[name]
        self.order_field = ORDER_FIELD[self.id] if name in BUILT_IN else register_modulus(self.c["n"], prime=True)
        self.G = (self.c["gx"], self.c["gy"])


@pytest.fixture(scope="module")
def spec():
    made = {}
    return lambda name: made.setdefault(name, Spec(name))


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def up8(engine, values):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint8)).to(engine.tdev)


def ints(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def points(engine, qx, qy):
    return list(zip(ints(engine, qx), ints(engine, qy)))


def recover_ints(engine, sp, e, r, s, v):
    qx, qy, ok = engine.ecdsa_recover(sp.id, up(engine, e), up(engine, r), up(engine, s), up8(engine, v))
    return points(engine, qx, qy), [int(b) for b in engine.to_numpy(ok)]


def host_valid(c, r, s, v):
    """ok of ecdsa_recover short of 'Q is finite': the ranges, x < p, and x^3 + a x + b a square (the model takes the root and squares it back;
    tests/test_ecdsa_recover_cpu.py holds that to Euler's criterion)."""
    x = r + (v >> 1) * c["n"]
    return v <= 3 and 1 <= r < c["n"] and 1 <= s < c["n"] and x < c["p"] and model.lift(c, r, v) is not None


def chain(engine, sp, e, r, s, v):
    """(qx, qy, ok) from the chain of existing calls, the refused lanes masked the way ecdsa_recover promises them: (0, 0), ok = 0."""
    qx, qy, fin, fits = model.chain_of_existing_calls(engine, sp.id, sp.order_field, sp.c, e, r, s, v)
    qx, qy, fin, fits = (engine.to_numpy(t) for t in (qx, qy, fin, fits))
    ri, si, vi = arr_to_ints(engine.to_numpy(r)), arr_to_ints(engine.to_numpy(s)), engine.to_numpy(v)
    valid = np.array([host_valid(sp.c, a, b, int(w)) for a, b, w in zip(ri, si, vi)], dtype=bool)
    assert not (valid & (fits == 0)).any()
    ok = valid & (fin != 0)
    qx, qy = qx.copy(), qy.copy()
    qx[~ok] = 0; qy[~ok] = 0
    return qx, qy, ok.astype(np.uint8), valid


# ---------------------------------------------------------------- 1. round trip against an independent implementation
@pytest.mark.parametrize("name", BUILT_IN)
def test_round_trip_against_libcrypto(engine, openssl, spec, name):
    sp = spec(name); c = sp.c; order = c["n"]
    n = 2048
    rng = np.random.default_rng(8100 + sp.id)
    rnd = lambda: ints_to_arr([to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)])
    d, k = rnd(), rnd()
    e = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    e[:6] = ints_to_arr([0, 1, order - 1, order, 2**256 - 1, 2**255])
    qx, qy, inf = openssl.scalar_mult_base(sp.id, d, threads=THREADS)
    kx, ky, kinf = openssl.scalar_mult_base(sp.id, k, threads=THREADS)
    assert not inf.any() and not kinf.any()
    E, D, K = (engine.to_device(t) for t in (e, d, k))
    r0, s0, ok0 = (engine.to_numpy(t) for t in engine.ecdsa_sign(sp.id, E, D, K))
    r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, E, D, K)
    assert np.array_equal(engine.to_numpy(r), r0) and np.array_equal(engine.to_numpy(s), s0) and np.array_equal(engine.to_numpy(ok), ok0) and ok0.all()
    want_v = np.array([(to_int(y) & 1) | (2 if to_int(x) >= order else 0) for x, y in zip(kx, ky)], dtype=np.uint8)
    assert np.array_equal(engine.to_numpy(v), want_v)
    gx, gy, gok = (engine.to_numpy(t) for t in engine.ecdsa_recover(sp.id, E, r, s, v))
    assert gok.all() and np.array_equal(gx, qx) and np.array_equal(gy, qy)
    x_only, none, xok = engine.ecdsa_recover(sp.id, E, r, s, v, x_only=True)                         # qy = NULL
    assert none is None and np.array_equal(engine.to_numpy(x_only), qx) and engine.to_numpy(xok).all()
    # the other root: r^-1 (-s R - e G), a different key that verifies too (it leads to -R, whose x is the same)
    ox, oy, ook = engine.ecdsa_recover(sp.id, E, r, s, v ^ 1)
    assert engine.to_numpy(ook).all() and not (np.all(engine.to_numpy(ox) == qx, axis=1) & np.all(engine.to_numpy(oy) == qy, axis=1)).any()
    assert engine.to_numpy(engine.ecdsa_verify(sp.id, E, r, s, ox, oy)).all()
    for i in range(16):
        ri, si, ei = to_int(r0[i]), to_int(s0[i]), to_int(e[i])
        u = pow(ri, -1, order)
        minus_R = (to_int(kx[i]), c["p"] - to_int(ky[i]))
        want = ec_add(sp.id, ec_mul(sp.id, (-ei * u) % order, sp.G), ec_mul(sp.id, si * u % order, minus_R))
        assert (to_int(engine.to_numpy(ox)[i]), to_int(engine.to_numpy(oy)[i])) == want
    # low s: every s <= n / 2, the same signature where it was low already, n - s and the flipped parity where not -- and still the signer's key
    rl, sl, vl, okl = engine.ecdsa_sign_recoverable(sp.id, E, D, K, low_s=True)
    s_int, sl_int = arr_to_ints(s0), ints(engine, sl)
    high = np.array([x > order // 2 for x in s_int])
    assert high.any() and (~high).any() and engine.to_numpy(okl).all() and np.array_equal(engine.to_numpy(rl), r0)
    assert all(b == (order - a if h else a) and b <= order // 2 for a, b, h in zip(s_int, sl_int, high))
    assert np.array_equal(engine.to_numpy(vl), want_v ^ high.astype(np.uint8))
    lx, ly, lok = (engine.to_numpy(t) for t in engine.ecdsa_recover(sp.id, E, rl, sl, vl))
    assert lok.all() and np.array_equal(lx, qx) and np.array_equal(ly, qy)
    assert openssl.ecdsa_verify(sp.id, e, engine.to_numpy(rl), engine.to_numpy(sl), qx, qy, threads=THREADS).all()


@pytest.mark.parametrize("name", ALL)
def test_round_trip_against_python_integers(engine, spec, name):
    """The leg that never skips, and the only one on registered curves: 64 lanes, every expected value from the host model."""
    sp = spec(name); c = sp.c
    rng = random.Random("round trip " + name)
    n = 64
    e = [rng.getrandbits(256) for _ in range(n)]
    d = [rng.randrange(1, c["n"]) for _ in range(n)]
    k = [rng.randrange(1, c["n"]) for _ in range(n)]
    d[5], k[6], k[7], d[8] = 0, 0, c["n"], c["n"] + 1                     # refused lanes: r = s = v = 0, nothing to recover
    Q = [model.ec_mul(c, x, sp.G) if 1 <= x < c["n"] else None for x in d]
    for low in (False, True):
        want = [model.sign_recoverable(c, a, b, w, low_s=low) for a, b, w in zip(e, d, k)]
        r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, up(engine, e), up(engine, d), up(engine, k), low_s=low)
        got = list(zip(ints(engine, r), ints(engine, s), [int(x) for x in engine.to_numpy(v)]))
        assert [int(x) for x in engine.to_numpy(ok)] == [int(w is not None) for w in want]
        assert got == [w if w is not None else (0, 0, 0) for w in want]
        r0, s0, ok0 = engine.ecdsa_sign(sp.id, up(engine, e), up(engine, d), up(engine, k))
        assert np.array_equal(engine.to_numpy(r0), engine.to_numpy(r)) and np.array_equal(engine.to_numpy(ok0), engine.to_numpy(ok))
        assert low or np.array_equal(engine.to_numpy(s0), engine.to_numpy(s))
        qx, qy, rok = engine.ecdsa_recover(sp.id, up(engine, e), r, s, v)
        assert [int(x) for x in engine.to_numpy(rok)] == [int(w is not None) for w in want]
        assert points(engine, qx, qy) == [q if w is not None else (0, 0) for q, w in zip(Q, want)]
        assert engine.to_numpy(engine.ecdsa_verify(sp.id, up(engine, e), r, s, qx, qy)).sum() == sum(w is not None for w in want)


# ---------------------------------------------------------------- 2. equal to the composition of existing calls
@pytest.mark.parametrize("name", BUILT_IN + ["brainpoolP256r1"])
def test_equals_the_chain_of_existing_calls(engine, spec, name):
    """2^16 random (e, r, s, v), r uniform below n -- about half of them are not x coordinates: Q and ok equal, bit for bit, what the public calls
    of the parent commit give when chained; ok equals the host's verdict (ranges and the Legendre symbol) wherever the sum is finite."""
    sp = spec(name); order = sp.c["n"]
    n = 1 << 16
    rng = np.random.default_rng(8200 + len(name))
    below = lambda: engine.to_device(ints_to_arr([to_int(x) % order for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)]))
    e, r, s = engine.to_device(rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)), below(), below()
    v = up8(engine, rng.integers(0, 4, size=n))
    want_x, want_y, want_ok, valid = chain(engine, sp, e, r, s, v)
    qx, qy, ok = (engine.to_numpy(t) for t in engine.ecdsa_recover(sp.id, e, r, s, v))
    assert 0.2 * n < valid.sum() < 0.4 * n                       # v < 2: about half are squares; v >= 2: x = r + n < p almost never
    assert np.array_equal(ok, want_ok) and np.array_equal(ok != 0, valid)          # (no infinite sum among random inputs)
    assert np.array_equal(qx, want_x) and np.array_equal(qy, want_y)
    assert engine.to_numpy(engine.ecdsa_verify(sp.id, e, r, s, engine.to_device(qx), engine.to_device(qy))).sum() == valid.sum()


# ---------------------------------------------------------------- 3. the second x candidate
@pytest.mark.parametrize("name, rs", [("p256", (3, 4, 6, 9)), ("secp256k1", (2, 4, 6, 7))])
def test_second_x_candidate(engine, spec, name, rs):
    sp = spec(name); c = sp.c; order, p = c["n"], c["p"]
    rng = random.Random("second x " + name)
    e, r, s, v, want = [], [], [], [], []
    for x_r in rs:
        for parity in (0, 1):
            R = model.lift(c, x_r, 2 | parity)
            assert R is not None and R[0] == x_r + order < p and R[1] & 1 == parity
            ei, si = rng.getrandbits(256), rng.randrange(1, order)
            u = pow(x_r, -1, order)
            Q = ec_add(sp.id, ec_mul(sp.id, si * u % order, R), ec_mul(sp.id, (-ei * u) % order, sp.G))
            e.append(ei); r.append(x_r); s.append(si); v.append(2 | parity); want.append(Q)
    got, ok = recover_ints(engine, sp, e, r, s, v)
    assert ok == [1] * len(want) and got == want
    Q = (up(engine, [q[0] for q in want]), up(engine, [q[1] for q in want]))
    assert engine.to_numpy(engine.ecdsa_verify(sp.id, up(engine, e), up(engine, r), up(engine, s), *Q)).all()
    # x = r + n >= p: refused, whatever r is worth as an x coordinate by itself
    big = [p - order, p - order + 1, p - order + 12345, order - 1, 2**255]
    got, ok = recover_ints(engine, sp, e[:5], big, s[:5], [2, 3, 2, 3, 2])
    assert ok == [0] * 5 and got == [(0, 0)] * 5


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("name", ALL)
def test_refusals_leave_their_neighbours_alone(engine, spec, name):
    sp = spec(name); c = sp.c; order = c["n"]
    rng = random.Random("refusals " + name)
    n = 128 * 6 + 17                                            # (one inversion per element at this size; test_large_shape_in_chunks has refusals inside shared inversions)
    d = [rng.randrange(1, order) for _ in range(n)]
    k = [rng.randrange(1, order) for _ in range(n)]
    e = [rng.getrandbits(256) for _ in range(n)]
    r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, up(engine, e), up(engine, d), up(engine, k))
    assert engine.to_numpy(ok).all()
    base = recover_ints(engine, sp, e, ints(engine, r), ints(engine, s), engine.to_numpy(v))
    assert base[1] == [1] * n
    r, s, v = ints(engine, r), ints(engine, s), [int(x) for x in engine.to_numpy(v)]
    off_curve = next(x for x in range(1, 1000) if not model.is_square(c, x))
    bad = {3: ("r", 0), 40: ("s", 0), 41: ("r", order), 130: ("s", order), 131: ("r", 2**256 - 1), 200: ("v", 4), 201: ("v", 255), 300: ("r", off_curve),
           301: ("s", 2**256 - 1), 302: ("v", 128 | v[302])}
    for i, (which, value) in bad.items():
        {"r": r, "s": s, "v": v}[which][i] = value
    # Q at infinity: R = k G, e = s k mod n
    kk, ss = rng.randrange(1, order), rng.randrange(1, order)
    kG = model.ec_mul(c, kk, sp.G)
    e[500], r[500], s[500], v[500] = ss * kk % order, kG[0] % order, ss, (kG[1] & 1) | (2 if kG[0] >= order else 0)
    assert model.front_end(c, e[500], r[500], s[500], v[500])[0] and model.recover(c, e[500], r[500], s[500], v[500]) is None
    # e >= n gives the key of e mod n: lane 600 carries e' in [n, 2^256), lane 601 the same signature with e' - n
    e[600] = rng.getrandbits(256) % (2**256 - order) + order
    e[601], r[601], s[601], v[601] = e[600] - order, r[600], s[600], v[600]
    e[602] = 0
    got, ok = recover_ints(engine, sp, e, r, s, v)
    refused = set(bad) | {500}
    assert ok == [int(i not in refused) for i in range(n)]
    for i in range(n):
        if i in refused:
            assert got[i] == (0, 0), i
        elif i not in (600, 601, 602):
            assert got[i] == base[0][i], i
    assert got[600] == got[601] != base[0][600]
    for i in list(refused) + [600, 601, 602]:
        assert model.recover(c, e[i], r[i], s[i], v[i]) == (None if i in refused else got[i]), i


# ---------------------------------------------------------------- 5. shapes
@pytest.mark.parametrize("name", BUILT_IN)
@pytest.mark.parametrize("n", [0, 1, 127, 129])
def test_small_shapes(engine, spec, name, n):
    sp = spec(name); order = sp.c["n"]
    rng = random.Random(n)
    e = [rng.getrandbits(256) for _ in range(n)]
    d = [rng.randrange(1, order) for _ in range(n)]
    k = [rng.randrange(1, order) for _ in range(n)]
    r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, up(engine, e).reshape(n, 4), up(engine, d).reshape(n, 4), up(engine, k).reshape(n, 4))
    qx, qy, rok = engine.ecdsa_recover(sp.id, up(engine, e).reshape(n, 4), r, s, v)
    assert int(engine.to_numpy(ok).sum()) == n and int(engine.to_numpy(rok).sum()) == n
    assert points(engine, qx, qy) == [model.ec_mul(sp.c, x, sp.G) for x in d]


@pytest.mark.parametrize("name", BUILT_IN)
def test_large_shape_in_chunks(engine, spec, name):
    """2^22 + 5 elements (two passes through the window loops, 128 elements per shared inversion), everything generated and compared on the device:
    sign, recover, then on ALL lanes the recovered key equals d G from the fixed-base comb and ecdsa_verify accepts it; on a strided sample of 4 096
    lanes (a cap on the oracle's cost, not on coverage) the chain of existing calls gives the same bits."""
    import torch
    from ecsimd_amd import OUT_AFFINE, ALG_WINDOWED
    sp = spec(name)
    n = (1 << 22) + 5
    e = engine.fill_random(n, 91, 1)
    d = engine.fill_random(n, 91, 2, clear_top_bits=1)                         # < 2^255 < n; zero has probability 2^-255
    k = engine.fill_random(n, 91, 3, clear_top_bits=1)
    r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, e, d, k, low_s=True)
    assert bool(ok.all()) and bool((v <= 3).all()) and bool((v == 0).any()) and bool((v == 1).any())
    v[7] = 4; r[8] = 0; s[n - 1] = -1                                          # three refusals, one of them in the second chunk's tail
    qx, qy, rok = engine.ecdsa_recover(sp.id, e, r, s, v)
    want_ok = torch.ones(n, dtype=torch.uint8, device=rok.device); want_ok[[7, 8, n - 1]] = 0
    assert torch.equal(rok, want_ok)
    px, py = engine.scalar_mult_base(sp.id, d, flags=OUT_AFFINE | ALG_WINDOWED)
    px[[7, 8, n - 1]] = 0; py[[7, 8, n - 1]] = 0
    assert torch.equal(qx, px) and torch.equal(qy, py)
    assert torch.equal(engine.ecdsa_verify(sp.id, e, r, s, qx, qy), want_ok)
    rows = np.unique(np.concatenate([np.arange(0, n, n // 4090), [7, 8, n - 1, n - 2, 1 << 22, (1 << 22) - 1]]))[:4096 + 8]
    pick = lambda t: engine.select_rows(t, rows)
    cx, cy, cok, _ = chain(engine, sp, pick(e), pick(r), pick(s), pick(v))
    assert np.array_equal(cx, engine.to_numpy(pick(qx))) and np.array_equal(cy, engine.to_numpy(pick(qy))) and np.array_equal(cok, engine.to_numpy(pick(rok)))


@pytest.mark.parametrize("name", ["p256", "secp256k1", "sm2"])
def test_aliased_outputs_are_refused_and_the_workspace_is_left_clean(engine, spec, name):
    sp = spec(name); order = sp.c["n"]
    n = 5000
    rng = np.random.default_rng(8500 + sp.id % 7)
    rnd = lambda: engine.to_device(ints_to_arr([to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)]))
    e, d, k = rnd(), rnd(), rnd()
    r, s, v, ok = engine.empty(n), engine.empty(n), engine.flags(n), engine.flags(n)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda r_, s_: engine.lib.ecsimd_hip_ecdsa_sign_recoverable(engine.ctx, C.c_int(sp.id), p(e), p(d), p(k), p(r_), p(s_), p(v), p(ok), C.c_size_t(n), C.c_int(0))
    for r_, s_ in ((k, s), (r, d), (e, s), (r, r), (r, k)):
        assert call(r_, s_) != 0
    assert engine.lib.ecsimd_hip_ecdsa_sign_recoverable(engine.ctx, C.c_int(sp.id), p(e), p(d), p(k), p(r), p(s), p(v), p(ok), C.c_size_t(n), C.c_int(2)) != 0   # unknown flag
    # the control shows that the readback sees what a call leaves behind; then the five arrays of the call (Jacobian k G, affine x AND y) read as zeros
    engine.double_scalar_mult(sp.id, e, d, *engine.scalar_mult_base(sp.id, k, flags=2 | 4))
    assert np.count_nonzero(engine.workspace_bytes()[:5 * n * 32]) > 2 * n * 32      # (a registered curve's plan starts with two arrays only the ladder route writes)
    r, s, v, ok = engine.ecdsa_sign_recoverable(sp.id, e, d, k)
    after = engine.workspace_bytes()
    used = 5 * n * 32 if name in BUILT_IN else 9 * n * 32                      # a registered curve: the nine arrays of its plan
    assert after.size >= used and not after[:used].any()
    assert bool(ok.all()) and bool((v <= 3).all()) and bool((engine.to_numpy(r) != 0).any())
