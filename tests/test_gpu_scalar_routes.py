"""GPU suite: every scalar-multiplication route over tests/scalar_catalogue.py, lane for lane against the big-int model (helpers.ec_mul).

The catalogue holds the scalars AIMED at the recodings' rare links -- on secp256k1 the rounding carry of the GLV split (2^-33 per random scalar),
abs256's borrow chain, the unsigned top digit, zero halves, one digit in every position -- next to the edge lists the parity tests already run.  The
public window loops saw those edges only against the ladder, the constant-time loops (their own table layout, zero-digit select and, on secp256k1,
the complete addition law) only against the public loops on eight of them.  Here each route answers to the integer group law on its own: a wrong
lane is named with the features its scalar was chosen for.  The ladder is not the witness: at its three degenerate scalars it is held to the oracle."""
import random

import numpy as np
import pytest

import scalar_catalogue as sc
from helpers import CURVE_PARAMS, P256, SECP256K1, SEED, from_int, ints_to_arr, arr_to_ints, ec_add, ec_mul
from ecsimd_amd import (OUT_AFFINE, BASE_MGRY, ALG_WINDOWED, ALG_WINDOWED_SIGNED, ALG_WINDOWED_BIG, ALG_CONSTANT_TIME, ALG_NO_ENDOMORPHISM)

pytestmark = pytest.mark.gpu
CURVES = [P256, SECP256K1]
WAVE = 64
WINDOW_ROUTES = ((ALG_WINDOWED, "windowed"), (ALG_WINDOWED | ALG_NO_ENDOMORPHISM, "windowed, no endomorphism"),
                 (ALG_WINDOWED | ALG_CONSTANT_TIME, "windowed, constant time"),
                 (ALG_WINDOWED | ALG_CONSTANT_TIME | ALG_NO_ENDOMORPHISM, "windowed, constant time, no endomorphism"))
_G_DOUBLES, _BATCH = {}, {}


def mul_g(cv, k):
    """k G on Python integers from the doubles of G (k already reduced)."""
    c = CURVE_PARAMS[cv]
    if cv not in _G_DOUBLES:
        t = [(c["gx"], c["gy"])]
        for _ in range(255):
            t.append(ec_add(cv, t[-1], t[-1]))
        _G_DOUBLES[cv] = t
    r = None
    for i, d in enumerate(_G_DOUBLES[cv]):
        if (k >> i) & 1:
            r = ec_add(cv, r, d)
    return r


def ints_of(engine, t):
    return arr_to_ints(engine.to_numpy(t))


def xy(pt):
    return pt or (0, 0)


def batch(engine, cv):
    """The catalogue in the first lanes, random scalars behind it up to whole waves plus 5 lanes (at least three waves); lane-distinct base points
    s_i G from the device; k_i P_i and k_i G from the model, once for every test of the module."""
    if cv in _BATCH:
        return _BATCH[cv]
    order = CURVE_PARAMS[cv]["n"]
    cat = sc.catalogue(cv)
    lanes = WAVE * max(3, -(-(len(cat) - 5 + 1) // WAVE)) + 5
    rng = random.Random(SEED + cv)
    ks = [k for k, _ in cat] + [rng.getrandbits(256) for _ in range(lanes - len(cat))]
    feats = [sorted(f) for _, f in cat] + [["random"]] * (lanes - len(cat))
    ss = [rng.randrange(1, order) for _ in range(lanes)]
    k = engine.to_device(ints_to_arr(ks))
    bx, by = engine.scalar_mult_base(cv, engine.to_device(ints_to_arr(ss)), flags=OUT_AFFINE)
    base = list(zip(ints_of(engine, bx), ints_of(engine, by)))
    assert base == [mul_g(cv, s) for s in ss], "the base points themselves"
    B = dict(n=lanes, ks=ks, feats=feats, k=k, bx=bx, by=by, base=base,
             exp=[xy(ec_mul(cv, kv % order, P)) for kv, P in zip(ks, base)], exp_g=[xy(mul_g(cv, kv % order)) for kv in ks],
             degenerate=[i for i, kv in enumerate(ks) if kv in sc.ladder_degenerate_scalars(cv)])
    assert lanes <= 1 << 12 and lanes % WAVE == 5 and lanes > len(cat)
    _BATCH[cv] = B
    return B


def wrong_lanes(B, want, gx, gy=None, skip=()):
    """The lanes whose point is not the model's, each with its scalar and the features it was chosen for; gy None: x only."""
    bad = [i for i in range(len(want)) if i not in skip and (gx[i] != want[i][0] or (gy is not None and gy[i] != want[i][1]))]
    return [(i, hex(B["ks"][i]), B["feats"][i]) for i in bad]


def held(B, name, want, x, y=None, skip=(), engine=None):
    """[] where the route gives the model's points, else one entry: (route, wrong lanes, their features together, the first four of them).  The tests
    gather these over their routes and assert once, so that a failure names every route that is wrong."""
    bad = wrong_lanes(B, want, ints_of(engine, x), None if y is None else ints_of(engine, y), skip)
    return [(name, len(bad), sorted({f for _, _, fs in bad for f in fs}), bad[:4])] if bad else []


def report(wrong):
    """One line per wrong route, whole (pytest shortens the repr of a list)."""
    return "\n" + "\n".join("  " + "; ".join(str(part) for part in entry) for entry in wrong)


def test_the_catalogue_copies_the_parity_tests_list(engine):
    from test_gpu_parity import comb_exceptional_scalars
    for cv in CURVES:
        assert sc.comb_exceptional_scalars(cv) == comb_exceptional_scalars(cv)


@pytest.mark.parametrize("cv", CURVES)
def test_variable_base_routes_over_the_catalogue(engine, oracle, cv):
    """scalar_mult: the four window routes (on secp256k1: k_varwin_mult_glv, k_varwin_mult_odd<false>, k_varwin_mult_glv_ct, k_varwin_mult_odd<true>; on P-256
    the odd-digit loop, public and constant-time, with and without the flag that means nothing there), each with a classical and a Montgomery-form base
    point, x only, and in place over the base point; the ladder beside them, held to the oracle at its degenerate scalars."""
    import torch
    B = batch(engine, cv)
    k, bx, by, want = B["k"], B["bx"], B["by"], B["exp"]
    P = engine.from_affine(cv, bx, by)
    wrong = []
    for alg, name in WINDOW_ROUTES:
        x, y = engine.scalar_mult(cv, k, bx, by, flags=OUT_AFFINE | alg)
        wrong += held(B, name, want, x, y, engine=engine)
        mx, my = engine.scalar_mult(cv, k, P[0], P[1], flags=OUT_AFFINE | alg | BASE_MGRY)
        wrong += held(B, name + ", Montgomery-form base", want, mx, my, engine=engine)
        xo, none = engine.scalar_mult(cv, k, bx, by, flags=OUT_AFFINE | alg, x_only=True)
        assert none is None
        wrong += held(B, name + ", x only", want, xo, engine=engine)
        ix, iy = bx.clone(), by.clone()
        engine.scalar_mult(cv, k, ix, iy, flags=OUT_AFFINE | alg, out=[ix, iy, None])
        wrong += held(B, name + ", in place", want, ix, iy, engine=engine)
    lx, ly = engine.scalar_mult(cv, k, bx, by, flags=OUT_AFFINE)
    wrong += held(B, "ladder", want, lx, ly, skip=B["degenerate"], engine=engine)
    assert not wrong, report(wrong)
    d = B["degenerate"]
    assert len(d) == 3
    rows = np.array(d)
    ox, oy = oracle.to_affine(cv, oracle.scalar_mult(cv, engine.to_numpy(k)[rows], engine.to_numpy(bx)[rows], engine.to_numpy(by)[rows], threads=1))
    assert np.array_equal(engine.to_numpy(lx)[rows], ox) and np.array_equal(engine.to_numpy(ly)[rows], oy), "ladder at its degenerate scalars"
    assert torch.equal(bx, B["bx"]) and torch.equal(by, B["by"])


def shared_scalar_list(cv):
    order = CURVE_PARAMS[cv]["n"]
    if cv == P256:
        return [1, 2, 8, order - 2, order - 1, order + 1, 2**256 - 1, 2**255, int("8" * 64, 16), 2**256 - order]
    cat = sc.catalogue(cv)
    first = lambda name: next(k for k, f in cat if name in f)
    return sc.with_feature(cv, "carry_") + [first(s) for s in ("sign_pp", "sign_pn", "sign_np", "sign_nn", "k1_zero", "k2_zero")] + [0, order]


@pytest.mark.parametrize("cv", CURVES)
def test_shared_scalar_form_over_the_chosen_scalars(engine, cv):
    """scalar_mult_1s (k_stride = 0: every lane reads the one scalar): on secp256k1 every carry_* scalar, one of each sign pair, a zero first and a zero
    second half, k = 0 and k = n; on P-256 ten edge scalars.  65 lanes each, P_i = (s + i) G, so that k P_i = k P_0 + i (k G) costs the model two products."""
    order = CURVE_PARAMS[cv]["n"]
    lanes = WAVE + 1
    s0 = random.Random(SEED + 11 + cv).randrange(1, order - lanes)
    bx, by = engine.scalar_mult_base(cv, engine.to_device(ints_to_arr([s0 + i for i in range(lanes)])), flags=OUT_AFFINE)
    P0 = mul_g(cv, s0)
    assert (ints_of(engine, bx)[0], ints_of(engine, by)[0]) == P0
    ks = shared_scalar_list(cv)
    assert len(ks) == (10 if cv == P256 else 18 + 6 + 2)
    wrong = []
    for kv in ks:
        step, pt, want = mul_g(cv, kv % order), ec_mul(cv, kv % order, P0), []
        for _ in range(lanes):
            want.append(xy(pt)); pt = ec_add(cv, pt, step)
        for alg, name in ((ALG_WINDOWED, "windowed"), (ALG_WINDOWED | ALG_CONSTANT_TIME, "windowed, constant time")):
            x, y = engine.scalar_mult_1s(cv, from_int(kv), bx, by, flags=OUT_AFFINE | alg)
            got = list(zip(ints_of(engine, x), ints_of(engine, y)))
            if got != want:
                wrong.append((name, hex(kv), sorted(dict(sc.catalogue(cv)).get(kv, ())), [i for i in range(lanes) if got[i] != want[i]][:4]))
    assert not wrong, report(wrong)


@pytest.mark.parametrize("cv", CURVES)
def test_generic_kernels_over_the_catalogue(engine, cv):
    """The built-in curve registered through the generic kernels: a second device opinion with no GLV split and no special prime, both window flags."""
    from ecsimd_amd.engine import register_curve
    c = CURVE_PARAMS[cv]
    gid = register_curve(c["p"], c["a"], c["b"], c["gx"], c["gy"], c["n"], generic_kernels=True)
    B = batch(engine, cv)
    wrong = []
    for alg, name in ((ALG_WINDOWED, "generic window loop"), (ALG_WINDOWED | ALG_CONSTANT_TIME, "generic window loop, constant time")):
        x, y = engine.scalar_mult(gid, B["k"], B["bx"], B["by"], flags=OUT_AFFINE | alg)
        wrong += held(B, name, B["exp"], x, y, engine=engine)
    assert not wrong, report(wrong)


@pytest.mark.parametrize("cv", CURVES)
def test_generator_combs_over_the_catalogue(engine, cv):
    """scalar_mult_base: the 5-bit constant-time comb every signing path shares, the 4-bit comb, the signed 7-bit comb and the 20-bit table, base G."""
    B = batch(engine, cv)
    wrong = []
    for alg, name in ((ALG_WINDOWED | ALG_CONSTANT_TIME, "5-bit comb, constant time"), (ALG_WINDOWED, "4-bit comb"), (ALG_WINDOWED_SIGNED, "signed 7-bit comb"),
                      (ALG_WINDOWED_BIG, "20-bit table")):
        x, y = engine.scalar_mult_base(cv, B["k"], flags=OUT_AFFINE | alg)
        wrong += held(B, name, B["exp_g"], x, y, engine=engine)
    assert not wrong, report(wrong)


def directed_scalars(cv):
    if cv == P256:
        return sorted(set(sc.edge_scalars(cv)))
    return sc.with_feature(cv, "carry_", "k1_zero", "k2_zero", "top1_", "neg_borrow_")


@pytest.mark.parametrize("cv", CURVES)
def test_the_split_behind_the_verification_calls(engine, cv):
    """Every call that ends in u1 G + u2 Q puts u2 -- never u1 -- through the variable-base window loop (capi.hip double_scalar_mult_impl: u1 G from the
    generator's table, u2 Q from varwin_scalar_mult without flags: k_varwin_mult_glv<4> on secp256k1, k_varwin_mult_odd<false> on P-256):
      double_scalar_mult, ecdsa_verify_rx   u2 as the caller passes it (256 bits, reduced by the loop);
      ecdsa_verify                          u2 = r / s, u1 = e / s;
      ecdsa_recover, eth_recover            u2 = s / r on the lifted R, u1 = -e / r.
    So a scalar T is forced into the loop by solving for the signature: verification -- R = u1 G + T (d G), r = R.x mod n, s = r / T, e = u1 s; recovery --
    R chosen, r = R.x, s = T r, e random.  T: every carry_*, k*_zero, top1_* and neg_borrow_* scalar of secp256k1, the edge list on P-256.  The calls must
    accept / return the model's key, and refuse e + 1.  schnorr_verify is left out: its u2 is n - H(R || P || m), a hash nobody can direct."""
    import torch
    c = CURVE_PARAMS[cv]; order = c["n"]
    Ts = directed_scalars(cv)
    feats = dict(sc.catalogue(cv))
    rng = random.Random(SEED + 21 + cv)
    m = len(Ts)
    assert m <= 1 << 12 and (cv == P256 or {p for p in ("carry_g1_w1", "carry_g2_w3", "k1_zero", "k2_zero", "top1_half1", "top1_half2", "neg_borrow_w3")} <=
                             set().union(*(feats[T] for T in Ts)))
    ds = [rng.randrange(1, order) for _ in range(m)]
    u1s = [rng.randrange(1, order) for _ in range(m)]
    Q = [mul_g(cv, d) for d in ds]
    R = [mul_g(cv, (u1 + T * d) % order) for u1, T, d in zip(u1s, Ts, ds)]
    up = lambda vals: engine.to_device(ints_to_arr(vals))
    wrong = []

    def note(what, lanes_):
        if len(lanes_):
            wrong.append((what, len(lanes_), sorted({f for i in lanes_ for f in feats[Ts[i]]}), [hex(Ts[i]) for i in lanes_][:4]))
    qx, qy = up([q[0] for q in Q]), up([q[1] for q in Q])
    # u1 G + T Q itself
    rx, ry, fin = engine.double_scalar_mult(cv, up(u1s), up(Ts), qx, qy)
    got = list(zip(ints_of(engine, rx), ints_of(engine, ry), engine.to_numpy(fin).tolist()))
    want = [(r[0], r[1], 1) if r else (0, 0, 0) for r in R]
    note("double_scalar_mult", [i for i in range(m) if got[i] != want[i]])
    # signatures built for T
    rows = [i for i in range(m) if Ts[i] % order and R[i] and R[i][0] % order]
    assert len(rows) >= m - 2                                                     # T = 0 and T = n have no inverse
    r_ = [R[i][0] % order for i in rows]
    s_ = [r * pow(Ts[i], -1, order) % order for r, i in zip(r_, rows)]
    e_ = [u1s[i] * s % order for s, i in zip(s_, rows)]
    sel = lambda vals: up([vals[i] for i in rows])
    vqx, vqy = sel([q[0] for q in Q]), sel([q[1] for q in Q])
    ok = engine.to_numpy(engine.ecdsa_verify(cv, up(e_), up(r_), up(s_), vqx, vqy))
    note("ecdsa_verify refuses a valid signature", [rows[j] for j in np.flatnonzero(ok == 0)])
    ok = engine.to_numpy(engine.ecdsa_verify(cv, up([(e + 1) % order for e in e_]), up(r_), up(s_), vqx, vqy))
    note("ecdsa_verify accepts e + 1", [rows[j] for j in np.flatnonzero(ok)])
    ok = engine.to_numpy(engine.ecdsa_verify_rx(cv, sel(u1s), sel(Ts), vqx, vqy, up(r_)))       # T as it is, above n where the catalogue says so
    note("ecdsa_verify_rx refuses a valid signature", [rows[j] for j in np.flatnonzero(ok == 0)])
    bumped = [(e + 1) * pow(s, -1, order) % order for e, s in zip(e_, s_)]
    ok = engine.to_numpy(engine.ecdsa_verify_rx(cv, up(bumped), sel(Ts), vqx, vqy, up(r_)))
    note("ecdsa_verify_rx accepts e + 1", [rows[j] for j in np.flatnonzero(ok)])
    # recovery with s / r = T
    ts = [rng.randrange(1, order) for _ in rows]
    Rr = [mul_g(cv, t) for t in ts]
    assert all(p[0] < order for p in Rr)                                        # (so that r = R.x and v has no "x >= n" bit)
    rr = [p[0] for p in Rr]
    sr = [Ts[i] * r % order for i, r in zip(rows, rr)]
    er = [rng.getrandbits(256) for _ in rows]
    v = torch.tensor([p[1] & 1 for p in Rr], dtype=torch.uint8, device=engine.tdev)
    keys = [xy(mul_g(cv, (-e * pow(r, -1, order) + Ts[i] * t) % order)) for e, r, i, t in zip(er, rr, rows, ts)]
    kx, ky, ok = engine.ecdsa_recover(cv, up(er), up(rr), up(sr), v)
    got = list(zip(ints_of(engine, kx), ints_of(engine, ky)))
    note("ecdsa_recover", [rows[j] for j in range(len(rows)) if got[j] != keys[j] or not engine.to_numpy(ok)[j]])
    if cv == SECP256K1:
        addr, kx, ky, ok = engine.eth_recover(up(er), up(rr), up(sr), v, want_key=True)
        got = list(zip(ints_of(engine, kx), ints_of(engine, ky)))
        note("eth_recover", [rows[j] for j in range(len(rows)) if got[j] != keys[j] or not engine.to_numpy(ok)[j]])
    assert not wrong, report(wrong)


def test_the_complete_addition_law_on_the_device(engine):
    """padd29 / pdbl29 (fe29.cuh; the arithmetic of k_varwin_mult_glv_ct alone) at the inputs a complete law exists for, through ecsimd_hip_fe29_raw on
    secp256k1: O + T, T + T through the ADDITION, T + (-T), 2T + T, 2 O and 2 T, T from five of the catalogue's scalars times G and in projective
    coordinates over a Z of no particular shape.  Limbs in and out by tools/radix29_model.py's conversions; the results are compared as points --
    affine, or O where Z = 0 mod p -- with the integer group law, not limb for limb."""
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import radix29_model as rm
    cv = SECP256K1
    p, order = CURVE_PARAMS[cv]["p"], CURVE_PARAMS[cv]["n"]
    RR = 1 << rm.RBITS
    enter = lambda v: rm.to_limbs(v * RR % p)
    leave = lambda limbs: rm.from_limbs(limbs) * pow(RR, -1, p) % p
    rng = random.Random(SEED + 31)
    cat = sc.catalogue(cv)
    pick = [next(k for k, f in cat if name in f) for name in ("carry_g1_w1", "carry_g2_w3", "neg_borrow_w2", "top1_half1", "digit_-8_everywhere")]
    Ts = [mul_g(cv, k % order) for k in pick]
    O = (0, 1, 0)

    def proj(pt):
        z = rng.randrange(1, p)
        return (pt[0] * z % p, pt[1] * z % p, z)
    neg = lambda pt: (pt[0], p - pt[1])
    adds, want_add, dbls, want_dbl = [], [], [], []
    for T in Ts:
        T2 = ec_add(cv, T, T)
        for A, Bp, W in ((O, T, T), (proj(T), T, T2), (proj(T), neg(T), None), (proj(T2), T, ec_add(cv, T2, T)), ((0, rng.randrange(1, p), 0), T, T)):
            adds.append([enter(v) for v in A + Bp]); want_add.append(W)
        for A, W in ((O, None), ((0, rng.randrange(1, p), 0), None), (proj(T), T2), ((T[0], T[1], 1), T2)):
            dbls.append([enter(v) for v in A]); want_dbl.append(W)

    def run(op, rows, want, name):
        inp = torch.tensor(np.array(rows, dtype=np.int64).astype(np.int32), device=engine.tdev).contiguous()
        out = engine.fe29_raw(1, op, inp).cpu().numpy()
        for j, (limbs, W) in enumerate(zip(out, want)):
            X, Y, Z = (leave([int(v) for v in coord]) for coord in limbs)
            if W is None:
                assert Z == 0 and Y != 0, (name, j, "expected the point at infinity (0 : Y : 0)")
                assert X == 0, (name, j)
            else:
                assert Z != 0, (name, j, "infinity where a finite point was expected")
                zi = pow(Z, -1, p)
                assert (X * zi % p, Y * zi % p) == W, (name, j)
    run(6, adds, want_add, "padd29")
    run(5, dbls, want_dbl, "pdbl29")
