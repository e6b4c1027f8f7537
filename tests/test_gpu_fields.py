"""GPU suite: the field layer for RUN-TIME moduli (k_gfield.hip) and the ECDSA verification built on it.

The reference's field layer is generic in the modulus type P (mgry_mul.h:84-121, mgry_csts.h:15-35, gfp.h:17-115).  Checked here:
  * every element-wise field entry point on a field id, against the oracle registered with the same modulus -- the five moduli the REAL
    reference is compiled for (oracle/ref_driver.cpp: both group orders, 2^255 - 19, 2^256 - 1, P-192's prime; the oracle is pinned to
    the reference on them by tests/test_oracle.py) and random odd moduli of every size;
  * the same against the compiled reference directly, where oracle/_ref exists;
  * the reference-square option on a run-time modulus against the compiled reference's own mgry_sqr;
  * ecsimd_hip_ecdsa_verify against libcrypto's ECDSA_do_verify on valid, tampered and malformed signatures, and its mod-n half
    against Python big-int arithmetic.
"""
import numpy as np
import pytest

from helpers import CURVE_PARAMS, P256, SECP256K1, R, from_int, to_int, ints_to_arr, arr_to_ints
from oracle.loader import REF_MODULI

pytestmark = pytest.mark.gpu
CURVES = [P256, SECP256K1]
THREADS = 16
PRIME_MODULI = {"n_p256", "n_secp256k1", "p25519", "p192"}


@pytest.fixture(scope="module")
def gpu(engine):
    from gpu_adapter import EngineNP
    return EngineNP(engine)


def field_id(p, prime=False):
    from ecsimd_amd.engine import register_modulus
    return register_modulus(p, prime=prime)


def operands(p, n, seed):
    rng = np.random.default_rng(seed)
    a = ints_to_arr([to_int(x) % p for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)])
    b = ints_to_arr([to_int(x) % p for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)])
    edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 2**32 - 1, 2**64 - 1, 2**128 - 1, 2**192 - 1, 2**255 - 1, 2**224, 2**96 - 1]
    edge = [v % p for v in edge]
    for i, v in enumerate(edge):
        a[i] = from_int(v); b[len(edge) - 1 - i] = from_int(v)
    a[20:40] = ints_to_arr([(p - 1 - j) % p for j in range(20)]); b[20:40] = ints_to_arr([(p - 1 - 3 * j) % p for j in range(20)])
    return a, b


def check_field(gpu, chk, fg, fc, p, n=4096, seed=1, prime=True, sqrt=True):
    """Every element-wise entry point on field id fg (HIP) against the checker `chk` on its id fc."""
    a, b = operands(p, n, seed)
    for name in ("mod_add", "mod_sub", "mgry_mul"):
        assert np.array_equal(getattr(gpu, name)(fg, a, b), getattr(chk, name)(fc, a, b)), (hex(p), name)
    assert np.array_equal(gpu.mgry_sqr(fg, a), chk.mgry_mul(fc, a, a)), hex(p)                      # the exact square (the reference's own defect: below)
    for name in ("mgry_from_classical", "mgry_to_classical"):
        assert np.array_equal(getattr(gpu, name)(fg, a), getattr(chk, name)(fc, a)), (hex(p), name)
    for cnt in (1, 2, 3, 9):
        assert np.array_equal(gpu.mod_shift_left(fg, a, cnt), chk.mod_shift_left(fc, a, cnt)), (hex(p), cnt)
    rng = np.random.default_rng(seed + 99)
    t8 = ints_to_arr([(to_int(x) % p) * (to_int(y) % 2**256) for x, y in zip(rng.integers(0, 2**64, size=(256, 4), dtype=np.uint64),
                                                                            rng.integers(0, 2**64, size=(256, 4), dtype=np.uint64))], 8)   # < p * 2^256
    t8[0] = 0; t8[1] = ints_to_arr([p * 2**256 - 1], 8)[0]; t8[2] = ints_to_arr([(p - 1) * (p - 1)], 8)[0]
    assert np.array_equal(gpu.mgry_reduce(fg, t8), chk.mgry_reduce(fc, t8)), hex(p)
    # classical product (an extension): against big-int arithmetic
    assert arr_to_ints(gpu.mod_mul(fg, a[:512], b[:512])) == [x * y % p for x, y in zip(arr_to_ints(a[:512]), arr_to_ints(b[:512]))]
    m = 300                                                                                          # > 256: the batched form takes more than one workgroup's lanes at m = 1
    assert np.array_equal(gpu.gfp_inverse(fg, a[:m]), chk.gfp_inverse(fc, a[:m])), hex(p)              # x^(p-2) in the checker; division steps here when prime
    if prime:
        am = arr_to_ints(a[:m]); Rm = R % p
        assert arr_to_ints(gpu.gfp_inverse(fg, a[:m])) == [(pow(v * pow(Rm, -1, p) % p, -1, p) * Rm % p) if v else 0 for v in am]
    e = from_int(0x1234567890abcdef_0fedcba987654321_00000000ffffffff_8000000000000001)
    assert np.array_equal(gpu.mgry_pow(fg, a[:64], e), chk.mgry_pow(fc, a[:64], e)), hex(p)
    for e in (from_int(0), from_int(1), from_int(2**255)):
        assert np.array_equal(gpu.mgry_pow(fg, a[:16], e), chk.mgry_pow(fc, a[:16], e))
    if sqrt and p % 4 == 3:
        sq = chk.mgry_mul(fc, a[:64], a[:64])
        s, ok = gpu.gfp_sqrt(fg, np.concatenate([sq, a[64:128]]))
        so, oko = chk.gfp_sqrt(fc, np.concatenate([sq, a[64:128]]))
        assert np.array_equal(ok, oko) and np.array_equal(s, so)
        assert np.array_equal(gpu.gfp_opposite(fg, a), chk.gfp_opposite(fc, a))


@pytest.mark.parametrize("name", sorted(REF_MODULI))
def test_runtime_modulus_vs_oracle(gpu, oracle, name):
    p = REF_MODULI[name]
    check_field(gpu, oracle, field_id(p, prime=name in PRIME_MODULI), oracle.register_modulus(p), p, prime=name in PRIME_MODULI, seed=len(name))


def test_runtime_moduli_vs_the_reference_fixtures(gpu, golden_moduli):
    """tests/golden/ref_moduli_vectors.json: vectors minted from the compiled reference for its five curve-less instances."""
    from test_oracle import check_moduli_fixtures
    check_moduli_fixtures(gpu, lambda p: field_id(p, prime=p != 2**256 - 1), golden_moduli)


def test_group_order_ids_are_built_in(engine, oracle):
    from ecsimd_amd.engine import P256_ORDER, SECP256K1_ORDER
    for cv, fid in ((P256, P256_ORDER), (SECP256K1, SECP256K1_ORDER)):
        n = CURVE_PARAMS[cv]["n"]
        assert field_id(n) == fid and to_int(engine.constant(fid, 0)) == n
        c = oracle.constants(oracle.register_modulus(n))
        for which, key in ((5, "r_p"), (6, "rsq_p"), (7, "pm1_r_p"), (10, "p_m2")):
            assert np.array_equal(engine.constant(fid, which), c[key])
    assert field_id(CURVE_PARAMS[P256]["p"]) == P256 and field_id(CURVE_PARAMS[SECP256K1]["p"]) == SECP256K1     # the curve primes keep their kernels


def test_random_odd_moduli_of_every_size(gpu, oracle):
    """Moduli nobody compiled anything for: random odd values of 2 .. 256 bits (composite almost surely -- Montgomery arithmetic needs
    p odd, not prime), registered WITHOUT the prime flag, so gfp_inverse is x^(p-2) bit by bit as gfp.h:42-44 writes it."""
    rng = np.random.default_rng(77)
    sizes = [2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 224, 254, 255, 256, 256, 256]
    for bits in sizes:
        p = (int.from_bytes(rng.bytes(32), "big") >> (256 - bits)) | (1 << (bits - 1)) | 1
        check_field(gpu, oracle, field_id(p), oracle.register_modulus(p), p, n=1024, seed=bits, prime=False, sqrt=(bits > 8))


@pytest.mark.parametrize("name", sorted(REF_MODULI))
def test_runtime_modulus_vs_the_live_reference(gpu, reference, name):
    """The compiled reference itself, instantiated for the same modulus (oracle/ref_driver.cpp fops<P>)."""
    p = REF_MODULI[name]
    fg, fr = field_id(p, prime=name in PRIME_MODULI), reference.register_modulus(p)
    a, b = operands(p, 2048, 5)
    for f in ("mod_add", "mod_sub", "mgry_mul"):
        assert np.array_equal(getattr(gpu, f)(fg, a, b), getattr(reference, f)(fr, a, b)), (name, f)
    for f in ("mgry_from_classical", "mgry_to_classical"):
        assert np.array_equal(getattr(gpu, f)(fg, a), getattr(reference, f)(fr, a)), (name, f)
    assert np.array_equal(gpu.mod_shift_left(fg, a, 5), reference.mod_shift_left(fr, a, 5))
    # random operands only: on the carry-heavy edge values the reference's x^(p-2) runs into its own square() defect (checked below in
    # compatibility mode, where the HIP path reproduces it)
    assert np.array_equal(gpu.gfp_inverse(fg, a[64:192]), reference.gfp_inverse(fr, a[64:192]))
    # the reference-square option: mgry_sqr with the reference's square() as written -- on carry-heavy operands, where it drops a carry
    pat = np.array([0, 0xffffffff, 0x80000000, 0x7fffffff, 1, 0xfffffffe], dtype=np.uint64)
    w = pat[np.random.default_rng(3).integers(0, len(pat), size=(4096, 8))]
    x = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).astype(np.uint64)
    x = ints_to_arr([v % p for v in arr_to_ints(x)])
    ref_sq = reference.mgry_sqr(fr, x)
    gpu.e.set_ref_square_compat(True)
    try:
        got = gpu.mgry_sqr(fg, x)
        inv_c = gpu.gfp_inverse(fg, x[:64])
    finally:
        gpu.e.set_ref_square_compat(False)
    assert np.array_equal(got, ref_sq), name
    assert np.array_equal(inv_c, reference.gfp_inverse(fr, x[:64])), name
    if p > 2**200:
        assert (ref_sq != reference.mgry_mul(fr, x, x)).any(axis=1).sum() > 0, "the sample never hit the reference's dropped carry"


def test_unknown_field_ids_are_refused(engine):
    import ctypes as C
    a = engine.to_device(ints_to_arr([1, 2, 3, 4]))
    out = engine.empty(4)
    for fid in (-1, 4096 + 2, 1 << 20):
        rc = engine.lib.ecsimd_hip_mgry_mul(engine.ctx, C.c_int(fid), C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), C.c_size_t(4))
        assert rc == -1
    p1 = field_id(2**255 - 19)                                       # = 1 mod 4: no GFp in the reference (gfp.h:84), no sqrt here
    ok = engine.flags(4)
    assert engine.lib.ecsimd_hip_gfp_sqrt(engine.ctx, C.c_int(p1), C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(ok.data_ptr()), C.c_size_t(4)) == -1


# ---------------------------------------------------------------- ECDSA
def signatures(openssl, cv, n, seed):
    order = CURVE_PARAMS[cv]["n"]
    rng = np.random.default_rng(seed)
    d = ints_to_arr([to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)])
    e = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)          # digests: any 256-bit value (most exceed neither n nor not)
    e[:8] = ints_to_arr([0, 1, order - 1, order, order + 1, 2**256 - 1, 2**255, 2**256 - order])
    r, s, qx, qy = openssl.ecdsa_sign(cv, d, e, threads=THREADS)
    return e, r, s, qx, qy


@pytest.mark.parametrize("cv", CURVES)
def test_ecdsa_verify_vs_libcrypto(engine, openssl, cv):
    """4 096 valid signatures made by libcrypto, then the same with each input tampered in turn, malformed (r, s) and invalid public keys:
    lane for lane the verdict of ECDSA_do_verify."""
    order = CURVE_PARAMS[cv]["n"]; p = CURVE_PARAMS[cv]["p"]
    n = 4096
    e, r, s, qx, qy = signatures(openssl, cv, n, 2024 + cv)
    up = engine.to_device
    run = lambda e_, r_, s_, x_, y_: engine.to_numpy(engine.ecdsa_verify(cv, up(e_), up(r_), up(s_), up(x_), up(y_)))
    assert run(e, r, s, qx, qy).all()
    rng = np.random.default_rng(9)
    # a mixed batch: every lane picks one way of being wrong (or none)
    kind = rng.integers(0, 12, size=n)
    e2, r2, s2, x2, y2 = (v.copy() for v in (e, r, s, qx, qy))
    for i in range(n):
        k = kind[i]
        if k == 1: e2[i, 0] ^= np.uint64(1)                                       # another message
        elif k == 2: r2[i] = from_int((to_int(r[i]) + 1) % order)                  # another r
        elif k == 3: s2[i] = from_int((to_int(s[i]) + 1) % order)                  # another s
        elif k == 4: x2[i], y2[i] = qx[(i + 1) % n], qy[(i + 1) % n]               # somebody else's key
        elif k == 5: r2[i] = from_int(0)                                           # r = 0
        elif k == 6: s2[i] = from_int(0)                                           # s = 0
        elif k == 7: r2[i] = from_int(to_int(r[i]) + order) if to_int(r[i]) + order < 2**256 else from_int(order)      # r >= n (r + n would verify without the range check)
        elif k == 8: s2[i] = from_int(order)                                       # s = n
        elif k == 9: y2[i] = from_int((to_int(qy[i]) + 1) % p)                     # a point off the curve
        elif k == 10: x2[i], y2[i] = from_int(0), from_int(0)                      # the point at infinity
        elif k == 11: s2[i] = from_int(order - to_int(s[i]))                       # (r, n - s): the other valid signature of the same message
    got = run(e2, r2, s2, x2, y2)
    exp = openssl.ecdsa_verify(cv, e2, r2, s2, x2, y2, threads=THREADS)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]
    assert exp[kind == 0].all() and exp[kind == 11].all() and not exp[(kind != 0) & (kind != 11)].any()
    # ragged sizes (one lane, one wave + 1, a workgroup + 1) and the empty batch
    for m in (0, 1, 65, 257):
        assert np.array_equal(run(e2[:m], r2[:m], s2[:m], x2[:m], y2[:m]), exp[:m])


@pytest.mark.parametrize("cv", CURVES)
def test_ecdsa_scalars_at_the_shared_inversion_sizes(engine, openssl, cv):
    """2^18 + 3 signatures: three elements share an inversion (one lane's strided slice), with invalid lanes among them --
    valid ones accepted, the tampered ones rejected; a libcrypto sample of 2 048 lanes agrees."""
    n = (1 << 18) + 3
    base = 4096
    e, r, s, qx, qy = signatures(openssl, cv, base, 31 + cv)
    rep = (n + base - 1) // base
    tile = lambda v: np.tile(v, (rep, 1))[:n].copy()
    E, Rr, S, X, Y = (tile(v) for v in (e, r, s, qx, qy))
    bad = np.arange(n) % 7 == 3
    S[bad] = 0                                                          # s = 0 inside shared-inversion groups
    worse = np.arange(n) % 11 == 5
    E[worse, 1] ^= np.uint64(0x10)
    up = engine.to_device
    got = engine.to_numpy(engine.ecdsa_verify(cv, up(E), up(Rr), up(S), up(X), up(Y)))
    assert np.array_equal(got == 1, ~(bad | worse))
    idx = np.random.default_rng(1).choice(n, 2048, replace=False)
    assert np.array_equal(got[idx], openssl.ecdsa_verify(cv, E[idx], Rr[idx], S[idx], X[idx], Y[idx], threads=THREADS))


@pytest.mark.parametrize("cv", CURVES)
def test_ecdsa_sign_leaves_no_nonce_derived_data_in_the_workspace(engine, cv):
    """VERDICT r4 next 5 / ADVICE r4: the Jacobian k G (X, Y, Z) and its affine x live in the context workspace during ecdsa_sign; the Z of an
    unnormalised k G together with the public r gives bits of the nonce away, and the block outlives the call.  After the call -- stream order, no
    extra synchronisation by the caller -- those 4 n elements read back as zeros; the control (the same comb through scalar_mult_base, which
    promises nothing of the kind) shows that the readback does see what a call leaves behind."""
    from ecsimd_amd import OUT_AFFINE, ALG_WINDOWED, ALG_CONSTANT_TIME
    order = CURVE_PARAMS[cv]["n"]
    n = 5000
    rng = np.random.default_rng(77 + cv)
    rnd = lambda: engine.to_device(ints_to_arr([to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)]))
    e, d, k = rnd(), rnd(), rnd()
    engine.scalar_mult_base(cv, k, flags=OUT_AFFINE | ALG_WINDOWED | ALG_CONSTANT_TIME)
    left = engine.workspace_bytes()
    assert left.size >= 3 * n * 32 and np.count_nonzero(left[:3 * n * 32]) > 2 * n * 32        # the control: a Jacobian k G is lying there
    r, s, ok = engine.ecdsa_sign(cv, e, d, k)
    after = engine.workspace_bytes()
    assert after.size >= 4 * n * 32 and not after[:4 * n * 32].any()
    assert bool(ok.all()) and bool((engine.to_numpy(r) != 0).any())


@pytest.mark.parametrize("cv", CURVES)
def test_ecdsa_sign_vs_big_ints_and_libcrypto(engine, openssl, cv):
    """ecsimd_hip_ecdsa_sign (k G on the constant-time comb, r and s on the order's field id): (r, s) equal the textbook formulas on Python
    integers with libcrypto's k G, libcrypto's ECDSA_do_verify and this library's own ecdsa_verify accept every one of them, out-of-range
    d / k are refused with r = s = 0 -- at a size where several signatures share an inversion too."""
    order = CURVE_PARAMS[cv]["n"]
    up = engine.to_device
    for n, seed in ((3001, 5), ((1 << 18) + 9, 6)):
        rng = np.random.default_rng(seed + cv)
        rnd = lambda: ints_to_arr([to_int(x) % (order - 1) + 1 for x in rng.integers(0, 2**64, size=(min(n, 4096), 4), dtype=np.uint64)])
        tile = lambda v: np.tile(v, ((n + len(v) - 1) // len(v), 1))[:n].copy()
        d, k = tile(rnd()), tile(rnd())
        e = tile(rng.integers(0, 2**64, size=(min(n, 4096), 4), dtype=np.uint64))
        e[:6] = ints_to_arr([0, 1, order - 1, order, 2**256 - 1, 2**255])
        bad = {10: ("d", 0), 11: ("d", order), 12: ("k", 0), 13: ("k", order), 14: ("k", order + 5), 15: ("d", 2**256 - 1)}
        for i, (which, v) in bad.items():
            (d if which == "d" else k)[i] = from_int(v)
        r, s, ok = (engine.to_numpy(t) for t in engine.ecdsa_sign(cv, up(e), up(d), up(k)))
        good = np.ones(n, dtype=bool); good[list(bad)] = False
        assert np.array_equal(ok == 1, good)
        assert not r[~good].any() and not s[~good].any()
        m = 2048                                                    # the textbook formulas on a sample, with libcrypto's k G
        idx = np.concatenate([np.arange(64), rng.choice(n, m - 64, replace=False)]); idx = idx[good[idx]]
        kx, _, inf = openssl.scalar_mult_base(cv, k[idx], threads=THREADS)
        assert not inf.any()
        for j, i in enumerate(idx):
            rr = to_int(kx[j]) % order
            ss = pow(to_int(k[i]), -1, order) * (to_int(e[i]) + rr * to_int(d[i])) % order
            assert (to_int(r[i]), to_int(s[i])) == (rr, ss), i
        qx, qy, _ = openssl.scalar_mult_base(cv, d[idx], threads=THREADS)
        assert openssl.ecdsa_verify(cv, e[idx], r[idx], s[idx], qx, qy, threads=THREADS).all()
        assert engine.to_numpy(engine.ecdsa_verify(cv, up(e[idx]), up(r[idx]), up(s[idx]), up(qx), up(qy))).all()
    if cv == P256:                                                  # RFC 6979 A.2.5, SHA-256, "sample": the nonce is the RFC's k
        x = 0xC9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721
        kk = 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60
        ee = 0xAF2BDBE1AA9B6EC1E2ADE1D694F41FC71A831D0268E9891562113D8A62ADD1BF
        r, s, ok = (engine.to_numpy(t) for t in engine.ecdsa_sign(cv, up(ints_to_arr([ee])), up(ints_to_arr([x])), up(ints_to_arr([kk]))))
        assert ok[0] == 1 and to_int(r[0]) == 0xEFD48B2AACB6A8FD1140DD9CD45E81D69D2C877B56AAF991C34D0EA84EAF3716
        assert to_int(s[0]) == 0xF7CB1C942D657C41D436C7A1B6E29F65F3E900DBB9AFF4064DC4AB2F843ACDA8


@pytest.mark.parametrize("cv", CURVES)
def test_ecdsa_sign_refuses_the_key_that_makes_s_zero(engine, cv):
    """r = x(k G) mod n comes from k alone, so d = -e / r mod n makes s = (e + r d) / k = 0: that lane is refused with r = s = 0, and its two neighbours
    d + 1, d - 1 are signed -- (r, s) of the textbook formulas with k G from the big-int curve model, and accepted by ecdsa_verify under d G."""
    from helpers import ec_mul
    c = CURVE_PARAMS[cv]; order = c["n"]; G = (c["gx"], c["gy"])
    rng = np.random.default_rng(40 + cv)
    draw = lambda: to_int(rng.integers(0, 2**64, size=4, dtype=np.uint64))
    e, d, k, want, pub = [], [], [], [], []
    for trip in range(6):
        ei, ki = draw(), draw() % (order - 1) + 1
        ri = ec_mul(cv, ki, G)[0] % order
        d0 = -ei * pow(ri, -1, order) % order
        assert ri != 0 and 2 <= d0 < order - 1 and (ei + ri * d0) % order == 0
        for di in (d0, d0 + 1, d0 - 1):
            si = pow(ki, -1, order) * (ei + ri * di) % order
            e.append(ei); d.append(di); k.append(ki); want.append((ri, si, 1) if si else (0, 0, 0)); pub.append(ec_mul(cv, di, G))
    assert [w[2] for w in want] == [0, 1, 1] * 6
    up = lambda values: engine.to_device(ints_to_arr(values))
    r, s, ok = (engine.to_numpy(t) for t in engine.ecdsa_sign(cv, up(e), up(d), up(k)))
    assert [(to_int(r[i]), to_int(s[i]), int(ok[i])) for i in range(len(want))] == want
    served = [i for i, w in enumerate(want) if w[2]]
    take = lambda values: up([values[i] for i in served])
    verdict = engine.ecdsa_verify(cv, take(e), take([w[0] for w in want]), take([w[1] for w in want]), take([q[0] for q in pub]), take([q[1] for q in pub]))
    assert engine.to_numpy(verdict).all()


@pytest.mark.parametrize("cv", CURVES)
def test_scalar_field_arithmetic_against_big_ints(gpu, cv):
    """u1 = e / s, u2 = r / s mod n by the public field entry points on the group-order field id: what ecdsa_verify computes inside."""
    from ecsimd_amd.engine import ORDER_FIELD
    order = CURVE_PARAMS[cv]["n"]; fid = ORDER_FIELD[cv]
    rng = np.random.default_rng(4 + cv)
    n = 1000
    ev = [int.from_bytes(rng.bytes(32), "big") % order for _ in range(n)]
    rv = [int.from_bytes(rng.bytes(32), "big") % order for _ in range(n)]
    sv = [int.from_bytes(rng.bytes(32), "big") % (order - 1) + 1 for _ in range(n)]
    sm = gpu.mgry_from_classical(fid, ints_to_arr(sv))
    wm = gpu.gfp_inverse(fid, sm)                                       # s^-1 R
    u1 = gpu.mgry_mul(fid, ints_to_arr(ev), wm)                         # e * (s^-1 R) / R
    u2 = gpu.mgry_mul(fid, ints_to_arr(rv), wm)
    assert arr_to_ints(u1) == [e * pow(s, -1, order) % order for e, s in zip(ev, sv)]
    assert arr_to_ints(u2) == [r * pow(s, -1, order) % order for r, s in zip(rv, sv)]


@pytest.mark.parametrize("p", [3, 5, 2**31 - 1, 2**61 - 1, 2**127 - 1, "n_p256", "n_secp256k1"])
def test_prime_flagged_moduli_through_the_shared_inversion(engine, oracle, p):
    """ecsimd_hip_register_modulus(p, PRIME) routes gfp_inverse to the shared division-step inversion (one per up to 128 elements).
    Small primes with canonical operands -- a third of them 0 for p = 3: a zero must come out as 0 WITHOUT zeroing the neighbours that share its
    inversion -- and, for the two group orders, ANY 256-bit operand (the reference never rejects a >= p, tests/ops.cpp:232; a = n and 2n - ... are 0
    as field elements): equal to the oracle's x^(p-2) (gfp.h:42-44) on every lane.  The same p registered WITHOUT the flag is another id and keeps
    the reference's power ladder (a later PRIME registration must not change it under its holder)."""
    from ecsimd_amd.engine import register_modulus
    big = isinstance(p, str)
    if big:
        p = CURVE_PARAMS[P256 if p == "n_p256" else SECP256K1]["n"]
    fid = register_modulus(p, prime=True)
    plain = register_modulus(p, prime=False)
    assert register_modulus(p, prime=True) == fid and register_modulus(p, prime=False) == plain
    assert big or fid != plain                                    # (the built-in order ids 2 / 3 are PRIME entries; an unflagged twin is a new id too)
    oid = oracle.register_modulus(p)
    n = (1 << 18) + 77
    rng = np.random.default_rng(p % 1000)
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    if big:
        a[:6] = ints_to_arr([0, p, 1, p - 1, p + 1, 2**256 - 1])
        a[1000:1064] = from_int(p)                                # a run of zeros-as-field-elements inside shared inversions
    else:
        a = ints_to_arr([to_int(x) % p for x in a[:4096]])
        a = np.tile(a, ((n + 4095) // 4096, 1))[:n].copy()
        a[:4] = ints_to_arr([0, 1, p - 1, p // 2])
    exp = oracle.gfp_inverse(oid, a)
    for f in (fid, plain):
        got = engine.to_numpy(engine.gfp_inverse(f, engine.to_device(a)))
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, (hex(p), f, bad[:8])
