"""The number-theoretic transform on the device (include/ecsimd_ntt.h) against tools/ntt_model.py's plain-integer definition: every size from 2 to 2^12 over
BLS12-381's scalar field at the default schedule and at ECSIMD_NTT_MAX_RADIX_LOG(1, 2, 3) -- two, three and many passes from four elements on --, cosets,
batches that share a workgroup and leave the last one ragged, in place against out of place, two other fields, a caller's root, the refusals, the bit
reversal, a polynomial product, the default schedule's smallest three-pass size, a captured forward - multiply - inverse chain, and the chain the feature
exists for: evaluations -> ntt_inverse -> g1_msm = a KZG commitment."""
import functools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ntt_model as model   # noqa: E402

pytestmark = pytest.mark.gpu
FR, FR_ROOT = model.FR, model.FR_ROOT
CAPS = (0, 1, 2, 3)                     # flags: the default schedule and ECSIMD_NTT_MAX_RADIX_LOG(1 .. 3)
TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def eng():
    from ecsimd_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def fr_field():
    from ecsimd_amd import Engine
    fid, root = Engine.ntt_bls12_381_fr()
    assert root == FR_ROOT
    return fid


_domains = {}


def domain(eng, field, log_n, root=None, shift=None):
    key = (id(eng), field, log_n, root, shift)
    if key not in _domains:
        _domains[key] = eng.ntt_domain(field, log_n, root, shift)
    return _domains[key]


def dev(eng, ints):
    a = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(len(ints), 4)
    return eng.to_device(a)


def host(eng, t):
    b = eng.to_numpy(t).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def arrays(p, n, seed):
    """The inputs of every comparison, as a batch: random values with 0, 1, p - 1 and values from p up to 2^256 - 1 among them; a constant array; a delta at 0, at 1
    and at n - 1."""
    rng = random.Random(seed)
    c = rng.randrange(p)
    delta = lambda i: [rng.randrange(1, p) if j == i else 0 for j in range(n)]
    return [model.edge_inputs(p, n, rng), [c] * n, delta(0), delta(1 % n), delta(n - 1)]


@functools.lru_cache(maxsize=None)
def reference(p, log_n, root, shift, seed, count=5):
    """(inputs, forward, inverse) of the batch, computed once and never changed"""
    xs = arrays(p, 1 << log_n, seed)[:count]
    return (tuple(map(tuple, xs)), tuple(tuple(model.forward(x, p, log_n, root, shift)) for x in xs), tuple(tuple(model.inverse(x, p, log_n, root, shift)) for x in xs))


def flat(rows):
    return [v for r in rows for v in r]


def check_transforms(eng, field, p, log_n, root, shift, seed, caps=CAPS, dom_root="same"):
    xs, fwd, inv = reference(p, log_n, root, shift, seed)
    dom = domain(eng, field, log_n, root if dom_root == "same" else dom_root, None if shift == 1 else shift)
    x = dev(eng, flat(xs))
    for flags in caps:
        assert host(eng, eng.ntt_forward(dom, x, flags=flags)) == flat(fwd), ("forward", log_n, flags)
        assert host(eng, eng.ntt_inverse(dom, x, flags=flags)) == flat(inv), ("inverse", log_n, flags)
        assert host(eng, eng.ntt_inverse(dom, dev(eng, flat(fwd)), flags=flags)) == [v % p for v in flat(xs)], ("inverse of forward", log_n, flags)
    one = dev(eng, list(xs[0]))                                               # ... and a batch of one
    assert host(eng, eng.ntt_forward(dom, one)) == list(fwd[0])


# ---- Fr
@pytest.mark.parametrize("log_n", range(1, 13))
def test_fr_every_size_at_every_schedule(eng, log_n):
    from ecsimd_amd import Engine
    check_transforms(eng, fr_field(), FR, log_n, FR_ROOT, 1, 100 + log_n)
    passes = [Engine.ntt_plan(log_n, 5, f)["passes"] for f in CAPS]
    assert passes == [-(-log_n // 9), log_n, -(-log_n // 2), -(-log_n // 3)]     # what the caps are for: the multi-pass code from four elements on


@pytest.mark.parametrize("log_n", (1, 5, 12))
def test_fr_on_a_coset(eng, log_n):
    check_transforms(eng, fr_field(), FR, log_n, FR_ROOT, 7, 200 + log_n)
    check_transforms(eng, fr_field(), FR, log_n, FR_ROOT, random.Random(log_n).randrange(2, FR), 300 + log_n)


@pytest.mark.parametrize("log_n", (1, 3, 6))
@pytest.mark.parametrize("batch", (1, 3, 67))
def test_batches_share_a_workgroup_and_leave_the_last_one_ragged(eng, log_n, batch):
    n, rng = 1 << log_n, random.Random(1000 * batch + log_n)
    xs = [model.edge_inputs(FR, n, rng) for _ in range(batch)]
    for shift in (1, 7):
        dom = domain(eng, fr_field(), log_n, FR_ROOT, None if shift == 1 else shift)
        fwd = flat(model.forward(x, FR, log_n, FR_ROOT, shift) for x in xs)
        for flags in CAPS:
            got = eng.ntt_forward(dom, dev(eng, flat(xs)), flags=flags)
            assert host(eng, got) == fwd, (log_n, batch, shift, flags)
            assert host(eng, eng.ntt_inverse(dom, got, flags=flags)) == [v % FR for v in flat(xs)], (log_n, batch, shift, flags)


@pytest.mark.parametrize("log_n", (3, 9, 10, 12))
def test_in_place_equals_out_of_place(eng, log_n):
    import torch
    xs, fwd, inv = reference(FR, log_n, FR_ROOT, 7, 400 + log_n)
    dom = domain(eng, fr_field(), log_n, FR_ROOT, 7)
    for flags in CAPS:
        for call, want in ((eng.ntt_forward, fwd), (eng.ntt_inverse, inv)):
            x = dev(eng, flat(xs)); keep = x.clone()
            apart = call(dom, x, flags=flags)
            assert torch.equal(x, keep), "an out-of-place call changed its input"
            same = call(dom, x, out=x, flags=flags)
            assert same.data_ptr() == x.data_ptr() and torch.equal(same, apart) and host(eng, same) == flat(want), (log_n, flags)


# ---- other fields, other roots
def test_a_field_of_low_two_adicity_and_a_dense_prime(eng):
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import register_modulus
    s, root = Engine.ntt_field_info(2)
    assert (s, root) == (model.two_adicity(model.P256_ORDER), model.default_root(model.P256_ORDER)) and s == 4
    check_transforms(eng, 2, model.P256_ORDER, 4, None, 1, 500)
    check_transforms(eng, 2, model.P256_ORDER, 4, None, 7, 501)
    dense = model.dense_prime()
    assert dense >> 224 == 0xffffffff and model.two_adicity(dense) >= 8
    fid = register_modulus(dense, prime=True)
    assert Engine.ntt_field_info(fid) == (model.two_adicity(dense), model.default_root(dense))
    check_transforms(eng, fid, dense, 8, None, 1, 502)
    check_transforms(eng, fid, dense, 8, None, dense - 2, 503)


def test_a_callers_root_and_the_default_root(eng):
    other = pow(FR_ROOT, 3, FR)                                              # an odd power of a primitive root is one
    assert other != model.default_root(FR) and model.is_root_of_order(other, 32, FR)
    check_transforms(eng, fr_field(), FR, 7, other, 1, 600, caps=(0, 2))
    check_transforms(eng, fr_field(), FR, 7, model.default_root(FR), 7, 601, caps=(0, 2), dom_root=None)     # NULL = the rule's root, which starts from 5
    xs, fwd, _ = reference(FR, 7, FR_ROOT, 1, 602)
    assert fwd != reference(FR, 7, other, 1, 602)[1]                          # the roots give different transforms of the same input


# ---- refusals
def test_refusals(eng):
    import torch
    from ecsimd_amd import Engine, EcsimdHipError
    fid = fr_field()
    for kw, word in ((dict(root=pow(FR_ROOT, 2, FR)), "root"), (dict(root=1), "root"), (dict(root=FR), "root"), (dict(root=FR_ROOT, shift=0), "shift"),
                     (dict(root=FR_ROOT, shift=FR), "shift"), (dict(root=FR_ROOT, shift=TOP), "shift")):
        with pytest.raises(EcsimdHipError, match=word):
            eng.ntt_domain(fid, 4, **kw)
    for log_n in (0, 25, 33):
        with pytest.raises(EcsimdHipError, match="log_n"):
            eng.ntt_domain(fid, log_n, FR_ROOT)
    with pytest.raises(EcsimdHipError, match="log_n"):
        eng.ntt_domain(2, 5)                                                 # s + 1 for P-256's order
    dom = domain(eng, fid, 4, FR_ROOT)
    buf = eng.empty(48)
    with pytest.raises(EcsimdHipError, match="overlap"):
        eng.ntt_forward(dom, buf[:32], out=buf[16:48])
    with pytest.raises(EcsimdHipError, match="overlap"):
        eng.ntt_inverse(dom, buf[8:24], out=buf[:16])
    with pytest.raises(EcsimdHipError, match="overlap"):
        eng.ntt_bitrev(4, buf[:32], out=buf[16:48])
    for flags in (10, 15, 16, -1):
        with pytest.raises(EcsimdHipError, match="flags"):
            eng.ntt_forward(dom, buf[:16], flags=flags)
    other = Engine(0)
    try:
        with pytest.raises(EcsimdHipError, match="another context"):
            other.ntt_forward(dom, other.empty(16))
    finally:
        other.close()
    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    said = []
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            try:
                eng.ntt_domain(fid, 5, FR_ROOT)
            except EcsimdHipError as e:
                said.append(str(e))
            eng.ntt_forward(dom, buf[:16], out=buf[:16])                     # the capture is still valid: a one-pass transform needs no warm-up
    torch.cuda.synchronize()
    assert len(said) == 1 and "capture" in said[0]
    del g


# ---- the permutation
@pytest.mark.parametrize("log_n", range(1, 13))
def test_bitrev(eng, log_n):
    import torch
    n, rng = 1 << log_n, random.Random(700 + log_n)
    xs = [[rng.getrandbits(256) for _ in range(n)] for _ in range(3)]
    x = dev(eng, flat(xs))
    want = flat(model.bitrev(r, log_n) for r in xs)
    out = eng.ntt_bitrev(log_n, x)
    assert host(eng, out) == want and host(eng, x) == flat(xs)
    assert host(eng, eng.ntt_bitrev(log_n, x[:n].contiguous())) == want[:n]
    same = eng.ntt_bitrev(log_n, x, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(same, out)


def test_poly_mul_equals_the_schoolbook_product(eng):
    rng = random.Random(800)
    a, b = [rng.randrange(FR) for _ in range(128)], [rng.randrange(FR) for _ in range(128)]
    school = [0] * 256
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            school[i + j] = (school[i + j] + u * v) % FR
    for shift in (None, 7):
        dom = domain(eng, fr_field(), 8, FR_ROOT, shift)
        assert host(eng, eng.ntt_poly_mul(dom, dev(eng, a + [0] * 128), dev(eng, b + [0] * 128))) == school


# ---- the default schedule's smallest three-pass size
def test_the_smallest_three_pass_transform(eng):
    import torch
    from ecsimd_amd import Engine
    log_n = next(L for L in range(1, 25) if Engine.ntt_plan(L)["passes"] == 3)
    assert log_n <= 22 and Engine.ntt_plan(log_n - 1)["passes"] == 2
    plan = Engine.ntt_plan(log_n)
    r1, r2, r3 = plan["log_radix"][:3]
    n = 1 << log_n
    assert plan["workspace_bytes"] == 32 * n and r1 + r2 + r3 == log_n
    dom = domain(eng, fr_field(), log_n, FR_ROOT)
    w = model.domain_omega(FR, log_n, FR_ROOT)
    rng = random.Random(900)
    # sparse: nonzero at 0, 1, n - 1 and on each side of the places where an input index changes its row in a pass (pass i reads row j at c + j n / 2^R_i)
    where = sorted({0, 1, n - 1, (n >> r1) - 1, n >> r1, (n >> r2) - 1, n >> r2, (n >> (r1 + r2)) - 1, n >> (r1 + r2), n // 2 - 1, n // 2})
    coeff = {i: rng.randrange(1, FR) for i in where}
    x = torch.zeros((n, 4), dtype=torch.int64, device=eng.tdev)
    x[torch.tensor(where, device=eng.tdev)] = dev(eng, [coeff[i] for i in where])
    got = eng.ntt_forward(dom, x)
    # outputs from every digit of every pass: output k = k1 + 2^R1 k2 + 2^(R1+R2) k3 is written by pass i from row k_i
    digits = lambda R: (0, 1, (1 << R) // 2, (1 << R) - 1)
    sample = sorted({k1 + (k2 << r1) + (k3 << (r1 + r2)) for k1 in digits(r1) for k2 in digits(r2) for k3 in digits(r3)} | {rng.randrange(n) for _ in range(64)})
    rows = host(eng, got[torch.tensor(sample, device=eng.tdev)])
    for k, v in zip(sample, rows):
        assert v == sum(c * pow(w, i * k, FR) for i, c in coeff.items()) % FR, k
    # dense: four outputs against Horner's rule, and the round trip on the device for all elements
    raw = np.random.default_rng(901).integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)      # below 2^254 < r: the round trip returns the very bytes
    xd = eng.to_device(raw)
    fwd = eng.ntt_forward(dom, xd)
    ints = host(eng, xd)
    ks = [0, 1, n - 1, rng.randrange(n)]
    for k, v in zip(ks, host(eng, fwd[torch.tensor(ks, device=eng.tdev)])):
        assert v == model.horner(ints, pow(w, k, FR), FR), k
    assert torch.equal(eng.ntt_inverse(dom, fwd), xd)
    assert torch.equal(eng.ntt_inverse(dom, fwd, out=fwd), xd)                # ... and in place: the first pass reads `out`, the last writes it


# ---- graph capture
def test_a_captured_forward_multiply_inverse_chain_replays(eng):
    import torch
    from ecsimd_amd import Engine
    log_n, batch = 8, 3
    n = 1 << log_n
    assert Engine.ntt_plan(log_n, batch)["workspace_bytes"] == 0             # one pass: capturable with no warm-up
    fresh = Engine(0)                                                        # a context that has run nothing
    try:
        dom = fresh.ntt_domain(fr_field(), log_n, FR_ROOT)
        rng = random.Random(1100)
        sets = [([rng.randrange(FR) for _ in range(batch * n)], [rng.randrange(FR) for _ in range(batch * n)]) for _ in range(3)]
        a, b = dev(fresh, sets[0][0]), dev(fresh, sets[0][1])
        torch.cuda.synchronize()
        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out = fresh.ntt_inverse(dom, fresh.mod_mul(fr_field(), fresh.ntt_forward(dom, a), fresh.ntt_forward(dom, b)))
        torch.cuda.synchronize()
        for xa, xb in sets[1:]:
            a.copy_(dev(fresh, xa)); b.copy_(dev(fresh, xb)); torch.cuda.synchronize()
            g.replay(); torch.cuda.synchronize()
            got = out.clone()
            eager = fresh.ntt_inverse(dom, fresh.mod_mul(fr_field(), fresh.ntt_forward(dom, a), fresh.ntt_forward(dom, b))); torch.cuda.synchronize()
            assert torch.equal(got, eager)
            want = []
            for t in range(batch):
                fa, fb = model.forward(xa[t * n:(t + 1) * n], FR, log_n, FR_ROOT), model.forward(xb[t * n:(t + 1) * n], FR, log_n, FR_ROOT)
                want += model.inverse([u * v % FR for u, v in zip(fa, fb)], FR, log_n, FR_ROOT)
            assert host(fresh, got) == want
        del g, out
        dom.close()
    finally:
        fresh.close()


# ---- the chain this exists for: evaluations over H -> coefficients -> a commitment
def test_evaluations_to_a_kzg_commitment(eng):
    import torch
    import bls12_381_model as bls
    log_n, n = 8, 256
    rng = random.Random(1200)
    tau = rng.randrange(2, FR)
    powers = [pow(tau, i, FR) for i in range(n)]
    gen = torch.from_numpy(np.frombuffer(bls.encode96(bls.G) * n, dtype=np.uint8).reshape(n, 96).copy()).to(eng.tdev)
    srs, ok = eng.bls12_381_g1_mul(dev(eng, powers), gen)
    assert bool(ok.all())
    evals = [rng.randrange(FR) for _ in range(n)]
    dom = domain(eng, fr_field(), log_n, FR_ROOT)
    coeffs = eng.ntt_inverse(dom, dev(eng, evals))                            # the transform's output IS the sum's scalar format
    commitment, finite = eng.bls12_381_g1_msm(coeffs, srs)
    p_tau = model.horner(model.inverse(evals, FR, log_n, FR_ROOT), tau, FR)
    want = bls.mul(p_tau, bls.G)
    assert int(finite.item()) == 1 and bytes(commitment.cpu().numpy()) == bls.encode96(want)
    got48, ok = eng.bls12_381_g1_compress(commitment.view(1, 96))
    assert bool(ok.all()) and bytes(got48.cpu().numpy()[0]) == bls.encode48(want)
