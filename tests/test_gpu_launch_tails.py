"""The refuse-or-reduce tails behind the hashes, run on the device with an order that reaches them.

BIP-32, BIP-340, the Taproot tweaks, RFC 6979's users and the recoverable signatures each end in a few select-only lines that decide whether a hash is usable
as a scalar modulo the group order n: IL < n, t < n, e mod n, n - e with 0 staying 0, k_child != 0, x(k G) >= n.  On secp256k1 a hash is at or above n with
probability 2^-128, so through the C ABI every lane the suite has ever run took the accepted side.  None of those kernels has the order compiled in: each takes
it as an argument (`words8 order` / `gmod M` in kernels.h).  tests/launch_probe.py calls the library's exported launchers one level below the C ABI, so the
library's own code objects run here with

  * N      the real order: the cases that become constructible once the inputs can be chosen after the digest is known (k_par = n - IL, d' = n - t,
           x(k G) in [n, p)), and the tie to the public API -- for every kernel one launch at N on ordinary inputs equals what the public entry point returns,
           which pins the probe's argument order (a wrapper bug would otherwise pass as a kernel finding);
  * HALF   one fixed odd constant between 2^255 and 3 * 2^254: about a third of the digests of a batch are on the refused side;
  * fitted orders: a lane's digest H itself (the lane sits AT n': refused, or e = 0), H + 2, H' + 1 (n' - 1: the largest accepted value), H' - 1 (n' + 1:
           refused, or reduced to 1).

What the kernels assume of an order, and what every surrogate order here respects: odd (Montgomery arithmetic modulo it) and 2^255 < n' < 2^256, so that a
256-bit value is below 2 n' -- reduce_once's one subtraction reduces it -- and g_add's operands are below n' once reduced.

Every expectation is tools/launch_tails_model.py's (hashlib / hmac and Python integers, the order a parameter; held to the suite's other models and the
published vectors by tests/test_launch_tails_cpu.py), every lane and every output array is compared, and what the test says of a batch -- so many lanes on
either side, this lane exactly at the order -- is asserted from the model before the device's answer is looked at.  Batches: tests/launch_tails_cases.py,
300 lanes (one workgroup and a partial one); messages of 32 bytes (contiguous), 45 bytes (odd stride and start) and 77 bytes twice (a whole block by word loads, and by byte loads from an odd start).

Launchers of kernels.h with an `order` / `gmod` parameter, taken: bip32_master, bip32_ckd_priv (both instantiations), bip32_ckd_pub_front (and _accept, which
has none but finishes the chain), schnorr_verify_front, schnorr_nonce, schnorr_finish, tweak_front (key path, Merkle root), taproot_seckey (with and without a
root), sign_recovery_id, ecdsa_sign_scalars, x_mod_n_equals / gc_x_mod_n_equals.  Left: rfc6979_nonce (its retry side is reached through the public API on
brainpoolP256r1: tests/test_gpu_ecdsa_deterministic.py), ecdsa_scalars and ecdsa_recover_scalars (range checks of caller-given r, s: reachable and tested
through ecdsa_verify / ecdsa_recover), recover_lift / gc_recover_lift (x = r + n < p is reachable with a chosen r: tests/test_gpu_ecdsa_recover.py),
gc_ladder_safe_scalars (tests/test_gpu_curves.py reaches its three scalars directly), tweak_front's TWEAK_GIVEN mode (t is the caller's: xonly_tweak_add with
t >= n is a public-API test), eth_recovery_id (`half` is an argument, s is the caller's), the gfield_* / gc_* arithmetic (any registered modulus reaches
them) and the comb kernels, whose `order` only recodes a scalar.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import launch_tails_cases as cases  # noqa: E402
import launch_tails_model as model  # noqa: E402
from ecsimd_amd.flags import OUT_AFFINE  # noqa: E402
from launch_probe import TWEAK_KEY_PATH, TWEAK_MERKLE_ROOT, Probe, device_to_ints, ints_to_device  # noqa: E402

pytestmark = pytest.mark.gpu
N, P, HALF, LANES = cases.N, cases.P, cases.HALF, cases.LANES
SECP256K1 = 1


@pytest.fixture(scope="module")
def probe(engine):
    return Probe(engine)


# ---- plumbing
def dev(engine, values):
    return ints_to_device(engine, values)


def dev_bytes(engine, values):
    return engine.torch.from_numpy(np.array(values, dtype=np.uint8)).to(engine.tdev)


def dev_index(engine, values):
    return engine.torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).to(engine.tdev)


def dev_messages(engine, batch, shape):
    """The messages as the column slice the batch describes: rows of shape[1] bytes, the message from column shape[2]."""
    nbytes, stride, first = shape
    whole = engine.torch.from_numpy(np.frombuffer(b"".join(batch["rows"]), dtype=np.uint8).reshape(LANES, stride).copy()).to(engine.tdev)
    view = whole[:, first:first + nbytes]
    assert view.data_ptr() == whole.data_ptr() + first and view.stride(0) == stride
    return view


def ints(t):
    return None if t is None else ([int(v) for v in t.cpu().numpy()] if t.dim() == 1 else device_to_ints(t))


def compare(what, got, want):
    """got: the output tensors of one launch; want: one tuple per lane from the model.  Every lane of every array."""
    cols = [ints(t) for t in got]
    assert all(len(c) == len(want) for c in cols)
    bad = [(i, j) for i, w in enumerate(want) for j in range(len(cols)) if cols[j][i] != w[j]]
    assert not bad, f"{what}: {len(bad)} values differ; first lanes (lane, output): {bad[:8]}; lane {bad[0][0]} got {[hex(c[bad[0][0]]) for c in cols]} want {[hex(v) for v in want[bad[0][0]]]}"


def orders_for(build, with_n=False):
    """[(label, n', batch)] for a batch builder: (N,) HALF and the four fitted orders, each with what the test says of it asserted from the model."""
    base = build(HALF)
    below, above = cases.sides(base["digest"], HALF)
    assert below >= cases.MIN_SIDE and above >= cases.MIN_SIDE, (below, above)       # a precondition on the seed, not on the kernel
    out = ([("N", N, build(N))] if with_n else []) + [("HALF", HALF, base)]
    if base["free"]:
        for n, lane, where in cases.fitted_orders(base):
            batch = build(n)
            cases.assert_placed(batch, n, lane, where)
            out.append((f"lane {lane} at n' {where:+d}", n, batch))
    return out


# ---- BIP-32
@pytest.mark.parametrize("seed_bytes", cases.SEED_BYTES)
def test_bip32_master(engine, probe, seed_bytes):
    for label, n, b in orders_for(lambda n: cases.master(seed_bytes), with_n=True):
        seeds = dev_bytes(engine, [list(s) for s in b["seed"]])
        got = probe.bip32_master(n, seeds)
        want = [model.bip32_master(n, s) for s in b["seed"]]
        if label == "HALF":
            assert sum(1 for w in want if w[2] == 0) >= cases.MIN_SIDE
        compare(f"bip32_master {seed_bytes} {label}", got, want)
        if label == "N":                             # the tie: the public entry point on the same seeds
            for g, e in zip(got, engine.bip32_master(seeds)):
                assert engine.torch.equal(g, e)


@pytest.mark.parametrize("with_point", [True, False])
def test_bip32_ckd_priv(engine, probe, with_point):
    for label, n, b in orders_for(lambda n: cases.ckd_priv(n, with_point), with_n=True):
        xP = dev(engine, [p[0] for p in b["point"]]) if with_point else None
        yP = dev(engine, [p[1] for p in b["point"]]) if with_point else None
        got = probe.bip32_ckd_priv(n, dev(engine, b["k"]), dev(engine, b["c"]), dev_index(engine, b["index"]), xP, yP, prime=n == N)
        want = [model.bip32_ckd_priv(n, b["k"][i], b["c"][i], b["index"][i], b["point"][i]) for i in range(LANES)]
        if with_point and label in ("N", "HALF"):    # the block of k_par = n' - IL (child key 0: refused) and its neighbours (served)
            block = [(i, want[i]) for i in cases.ZERO_BLOCK if b["digest"][i] < n]
            assert sum(1 for i, w in block if (i - cases.ZERO_BLOCK.start) % 3 == 0 and w == (0, 0, 0)) >= 3
            assert sum(1 for i, w in block if (i - cases.ZERO_BLOCK.start) % 3 != 0 and w[2] == 1 and w[0] in (1, n - 1)) >= 6
        compare(f"bip32_ckd_priv {with_point} {label}", got, want)
    # the tie: ordinary keys, the parent's point from scalar_mult_base, against the public entry point
    rng = np.random.default_rng(11)
    ks = [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES)]
    index = [int(v) | (model.HARDENED if with_point and i % 2 else 0) | (0 if with_point else model.HARDENED) for i, v in enumerate(rng.integers(0, 2**31, LANES))]
    k, c, idx = dev(engine, ks), dev(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)]), dev_index(engine, index)
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2] if with_point else (None, None)
    got = probe.bip32_ckd_priv(N, k, c, idx, qx, qy, prime=True)
    assert bool(got[2].all())
    for g, e in zip(got, engine.bip32_ckd_priv(k, c, idx, all_hardened=not with_point)):
        assert engine.torch.equal(g, e)


def test_bip32_ckd_pub_front(engine, probe):
    for label, n, b in orders_for(lambda n: cases.ckd_pub_front()):
        got = probe.bip32_ckd_pub_front(n, dev(engine, b["qx"]), dev(engine, b["qy"]), dev(engine, b["c"]), dev_index(engine, b["index"]))
        want = [model.bip32_ckd_pub_front(n, b["qx"][i], b["qy"][i], b["c"][i], b["index"][i]) for i in range(LANES)]
        if label == "HALF":                          # each cause of valid = 0 alone, and together with t >= n'
            seen = {(b["index"][i] >= model.HARDENED, not model.on_curve(b["qx"][i], b["qy"][i]), b["digest"][i] >= n) for i in range(LANES)}
            assert len(seen) == 8
        compare(f"bip32_ckd_pub_front {label}", got, want)
    # the tie: points of the curve at N; the front's t and K give the public entry point's child key, its c_child and valid the public c_child and ok
    rng = np.random.default_rng(12)
    k = dev(engine, [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES)])
    c = dev(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)])
    idx = dev_index(engine, [int(v) for v in rng.integers(0, 2**31, LANES)])
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    x, y, t, cc, valid = probe.bip32_ckd_pub_front(N, qx, qy, c, idx)
    cx, cy, pub_cc, ok = engine.bip32_ckd_pub(qx, qy, c, idx)
    assert bool(valid.all()) and engine.torch.equal(valid, ok) and engine.torch.equal(cc, pub_cc) and engine.torch.equal(x, qx) and engine.torch.equal(y, qy)
    tx, ty = engine.scalar_mult_base(SECP256K1, t, OUT_AFFINE)[:2]
    sx, sy, finite = engine.affine_add(SECP256K1, (x, y), (tx, ty))
    assert bool(finite.all()) and engine.torch.equal(sx, cx) and engine.torch.equal(sy, cy)
    one = dev(engine, [1] * LANES)
    for g, e in zip(probe.bip32_ckd_pub_accept(sx, sy, one, valid, cc.clone()), (cx, cy, pub_cc, ok)):
        assert engine.torch.equal(g, e)


def test_bip32_ckd_pub_accept(engine, probe):
    b = cases.ckd_pub_accept()
    want = [model.bip32_ckd_pub_accept(b["ax"][i], b["ay"][i], b["jz"][i], b["valid"][i], b["c"][i]) for i in range(LANES)]
    assert {(b["jz"][i] != 0, b["valid"][i] != 0) for i in range(LANES)} == {(False, False), (False, True), (True, False), (True, True)}
    assert all(v != 0 for v in b["c"])               # the pattern c_child is pre-filled with: cleared exactly where ok = 0, kept elsewhere
    got = probe.bip32_ckd_pub_accept(dev(engine, b["ax"]), dev(engine, b["ay"]), dev(engine, b["jz"]), dev_bytes(engine, b["valid"]), dev(engine, b["c"]))
    compare("bip32_ckd_pub_accept", got, want)


# ---- BIP-340
@pytest.mark.parametrize("shape", cases.MSG_SHAPES, ids=lambda s: f"{s[0]}B+{s[2]}")
def test_schnorr_verify_front(engine, probe, shape):
    for label, n, b in orders_for(lambda n: cases.verify_front(n, shape), with_n=True):
        got = probe.schnorr_verify_front(n, dev(engine, b["px"]), dev(engine, b["r"]), dev(engine, b["s"]), dev_messages(engine, b, shape))
        want = [model.schnorr_verify_front(n, b["px"][i], b["r"][i], b["s"][i], b["msgs"][i]) for i in range(LANES)]
        if label.endswith("+0"):                     # e = 0: u2 = 0, not n'
            lane = int(label.split()[1])
            assert want[lane][1] == 0 and want[lane][4] == 1
        if label == "HALF":
            assert sum(1 for i, w in enumerate(want) if w[4] == 1 and b["digest"][i] >= n) >= 32      # valid lanes whose challenge was reduced
        compare(f"schnorr_verify_front {shape} {label}", got, want)


def test_schnorr_verify_front_equals_the_public_api(engine, probe):
    rng = np.random.default_rng(13)
    d = dev(engine, [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES)])
    msgs = engine.torch.from_numpy(rng.integers(0, 256, (LANES, 45), dtype=np.uint8)).to(engine.tdev)
    px, r, s, ok = engine.schnorr_sign(d, msgs)
    assert bool(ok.all())
    s = s.clone(); s[::5, 0] ^= 1                    # every fifth signature spoiled
    u1, u2, x, y, valid = probe.schnorr_verify_front(N, px, r, s, msgs)
    rx, ry, finite = engine.double_scalar_mult(SECP256K1, u1, u2, x, y)
    verdict = finite.bool() & (rx == r).all(dim=1) & ((ry[:, 0] & 1) == 0) & valid.bool()
    public = engine.schnorr_verify(px, msgs, r, s).bool()
    assert bool(valid.all()) and engine.torch.equal(verdict, public) and int(public.sum()) == LANES - len(range(0, LANES, 5))


@pytest.mark.parametrize("shape", cases.MSG_SHAPES, ids=lambda s: f"{s[0]}B+{s[2]}")
def test_schnorr_nonce(engine, probe, shape):
    with_aux = shape[0] != 32                        # aux = NULL with the 32-byte messages, an aux array with the others
    for label, n, b in orders_for(lambda n: cases.nonce(n, shape, with_aux)):
        aux = dev(engine, b["aux"]) if with_aux else None
        got = probe.schnorr_nonce(n, dev(engine, b["d"]), aux, dev(engine, b["px"]), dev(engine, b["py"]), dev_messages(engine, b, shape))
        want = [(model.schnorr_nonce(n, b["d"][i], b["aux"][i], b["px"][i], b["py"][i], b["msgs"][i]),) for i in range(LANES)]
        if label == "HALF":
            served = [i for i in range(LANES) if 1 <= b["d"][i] < n]
            assert sum(1 for i in served if b["digest"][i] >= n) >= 32 and {b["py"][i] & 1 for i in served} == {0, 1} and want[0] == want[1] == (0,)
        compare(f"schnorr_nonce {shape} {label}", (got,), want)


@pytest.mark.parametrize("shape", cases.MSG_SHAPES, ids=lambda s: f"{s[0]}B+{s[2]}")
def test_schnorr_finish(engine, probe, shape):
    for label, n, b in orders_for(lambda n: cases.finish(n, shape), with_n=True):
        args = [dev(engine, b[k]) for k in ("d", "k0", "xP", "yP", "xR", "yR")]
        want = [model.schnorr_finish(n, b["d"][i], b["k0"][i], b["xP"][i], b["yP"][i], b["xR"][i], b["yR"][i], b["msgs"][i]) for i in range(LANES)]
        assert sum(1 for w in want if w[3] == 0) == 30 and {(b["yP"][i] & 1, b["yR"][i] & 1) for i in range(LANES)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        compare(f"schnorr_finish {shape} {label}", probe.schnorr_finish(n, *args, dev_messages(engine, b, shape), prime=n == N), want)
        px, r, s, ok = probe.schnorr_finish(n, *args, dev_messages(engine, b, shape), want_px=False, prime=n == N)
        assert px is None
        compare(f"schnorr_finish {shape} {label} without px", (r, s, ok), [w[1:] for w in want])


@pytest.mark.parametrize("with_aux", [False, True])
def test_schnorr_nonce_and_finish_equal_the_public_api(engine, probe, with_aux):
    rng = np.random.default_rng(14)
    d = dev(engine, [0, N] + [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES - 2)])
    aux = dev(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)]) if with_aux else None
    msgs = engine.torch.from_numpy(rng.integers(0, 256, (LANES, 32 if with_aux else 45), dtype=np.uint8)).to(engine.tdev)
    xP, yP = engine.scalar_mult_base(SECP256K1, d, OUT_AFFINE)[:2]
    k0 = probe.schnorr_nonce(N, d, aux, xP, yP, msgs)
    xR, yR = engine.scalar_mult_base(SECP256K1, k0, OUT_AFFINE)[:2]
    got = probe.schnorr_finish(N, d, k0, xP, yP, xR, yR, msgs, prime=True)
    want = engine.schnorr_sign(d, msgs, aux)
    assert ints(want[3]) == [0, 0] + [1] * (LANES - 2)
    for g, e in zip(got, want):
        assert engine.torch.equal(g, e)


# ---- Taproot
@pytest.mark.parametrize("has_root", [False, True])
def test_tweak_front(engine, probe, has_root):
    mode = TWEAK_MERKLE_ROOT if has_root else TWEAK_KEY_PATH
    for label, n, b in orders_for(lambda n: cases.tweak_front(has_root), with_n=True):
        px, merkle = dev(engine, b["px"]), (dev(engine, b["merkle"]) if has_root else None)
        got = probe.tweak_front(n, mode, px, merkle)
        want = [model.tweak_front(n, b["px"][i], b["merkle"][i]) for i in range(LANES)]
        if label == "HALF":                          # no lift alone, t >= n' alone, both
            assert len({(model.lift_even(b["px"][i]) is None, b["digest"][i] >= n) for i in range(LANES)}) == 4
        compare(f"tweak_front {has_root} {label}", got, want)
        if label == "N":                             # the tie: xonly_tweak_add of the front's t is the public taproot_tweak_pubkey
            x, y, t, valid = got
            for g, e in zip(engine.xonly_tweak_add(px, t), engine.taproot_tweak_pubkey(px, merkle)):
                assert engine.torch.equal(g, e)
            assert engine.torch.equal(valid, engine.taproot_tweak_pubkey(px, merkle)[2])


@pytest.mark.parametrize("has_root", [False, True])
def test_taproot_seckey(engine, probe, has_root):
    for label, n, b in orders_for(lambda n: cases.taproot_seckey(n, has_root), with_n=True):
        d, xP, yP, merkle = dev(engine, b["d"]), dev(engine, b["xP"]), dev(engine, b["yP"]), (dev(engine, b["merkle"]) if has_root else None)
        want = [model.taproot_seckey(n, b["d"][i], b["merkle"][i], b["xP"][i], b["yP"][i]) for i in range(LANES)]
        if label in ("N", "HALF"):                   # the block of d' = n' - t (sum 0: refused) and its neighbours (served), yP of both parities
            block = [(i, want[i]) for i in cases.ZERO_BLOCK if b["digest"][i] < n]
            zeros = [i for i, w in block if (i - cases.ZERO_BLOCK.start) % 3 == 0 and w == (0, 0, 0)]
            assert len(zeros) >= 3 and {b["yP"][i] & 1 for i in zeros} == {0, 1} and all(1 <= b["d"][i] < n for i in zeros)
            assert sum(1 for i, w in block if (i - cases.ZERO_BLOCK.start) % 3 != 0 and w[2] == 1 and w[0] in (1, n - 1)) >= 6
        compare(f"taproot_seckey {has_root} {label}", probe.taproot_seckey(n, d, merkle, xP, yP, prime=n == N), want)
        d_out, px, ok = probe.taproot_seckey(n, d, merkle, xP, yP, want_px=False, prime=n == N)
        assert px is None
        compare(f"taproot_seckey {has_root} {label} without px", (d_out, ok), [(w[0], w[2]) for w in want])
    rng = np.random.default_rng(15)                  # the tie
    d = dev(engine, [0, N] + [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES - 2)])
    merkle = dev(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)]) if has_root else None
    xP, yP = engine.scalar_mult_base(SECP256K1, d, OUT_AFFINE)[:2]
    for g, e in zip(probe.taproot_seckey(N, d, merkle, xP, yP, prime=True), engine.taproot_tweak_seckey(d, merkle)):
        assert engine.torch.equal(g, e)


# ---- ECDSA
@pytest.mark.parametrize("low_s", [False, True])
def test_sign_recovery_id(engine, probe, low_s):
    b = cases.recovery_id()
    want = [model.sign_recovery_id(N, b["x"][i], b["y"][i], b["s"][i], b["ok"][i], low_s) for i in range(LANES)]
    assert {w[1] for w in want} == {0, 1, 2, 3} and {(N - 1) // 2, (N + 1) // 2, 1, N - 1} <= set(b["s"]) and {N - 1, N, N + 1, P - 1} <= set(b["x"])
    got = probe.sign_recovery_id(N, dev(engine, b["x"]), dev(engine, b["y"]), dev(engine, b["s"]), dev_bytes(engine, b["ok"]), low_s)
    compare(f"sign_recovery_id low_s={low_s}", got, want)


def test_ecdsa_sign_scalars(engine, probe):
    b = cases.sign_scalars()
    want = [model.ecdsa_sign_scalars(N, b["e"][i], b["d"][i], b["k"][i], b["x"][i]) for i in range(LANES)]
    assert sum(1 for i, w in enumerate(want) if b["x"][i] > N and w == (b["x"][i] - N, w[1], 1)) >= 50           # r = x - n
    assert sum(1 for i, w in enumerate(want) if b["x"][i] == N and w == (0, 0, 0)) >= 10                         # r = 0
    triples = [want[i:i + 3] for i in range(100, 160, 3)]
    assert sum(1 for t in triples if t[0] == (0, 0, 0) and t[1][2] == 1 and t[2][2] == 1) >= 15                   # s = 0 between two served neighbours
    got = probe.ecdsa_sign_scalars(N, *(dev(engine, b[k]) for k in ("e", "d", "k", "x")))
    compare("ecdsa_sign_scalars", got, want)


@pytest.mark.parametrize("low_s", [False, True])
def test_sign_scalars_and_recovery_id_equal_the_public_api(engine, probe, low_s):
    rng = np.random.default_rng(16)
    draw = lambda: dev(engine, [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES)])
    e, d, k = dev(engine, [int.from_bytes(rng.bytes(32), "big") for _ in range(LANES)]), draw(), draw()
    x, y = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    r, s, ok = probe.ecdsa_sign_scalars(N, e, d, k, x)
    s, v = probe.sign_recovery_id(N, x, y, s, ok, low_s)
    for g, w in zip((r, s, v, ok), engine.ecdsa_sign_recoverable(SECP256K1, e, d, k, low_s=low_s)):
        assert engine.torch.equal(g, w)
    assert bool(ok.all())


def test_x_mod_n_equals(engine, probe):
    b = cases.x_mod_n()
    want = [(model.x_mod_n_equals(N, b["x"][i], b["finite"][i], b["r"][i]),) for i in range(LANES)]
    assert sum(1 for i, w in enumerate(want) if w == (1,) and b["x"][i] >= N) >= 20 and sum(1 for i, w in enumerate(want) if w == (0,) and b["x"][i] >= N and b["finite"][i]) >= 20
    x, r, finite = dev(engine, b["x"]), dev(engine, b["r"]), dev_bytes(engine, b["finite"])
    compare("x_mod_n_equals", (probe.x_mod_n_equals(SECP256K1, x, finite, r),), want)
    compare("gc_x_mod_n_equals", (probe.gc_x_mod_n_equals(N, x, finite, r),), want)
    # the tie: ecdsa_verify_rx is double_scalar_mult and this comparison
    rng = np.random.default_rng(17)
    draw = lambda: dev(engine, [1 + int.from_bytes(rng.bytes(32), "big") % (N - 1) for _ in range(LANES)])
    u1, u2, k = draw(), draw(), draw()
    qx, qy = engine.scalar_mult_base(SECP256K1, k, OUT_AFFINE)[:2]
    rx, _, fin = engine.double_scalar_mult(SECP256K1, u1, u2, qx, qy)
    rr = dev(engine, [v % N if i % 2 else (v + 1) % N for i, v in enumerate(ints(rx))])
    public = engine.ecdsa_verify_rx(SECP256K1, u1, u2, qx, qy, rr)
    assert ints(public) == [i % 2 for i in range(LANES)]
    assert engine.torch.equal(probe.x_mod_n_equals(SECP256K1, rx, fin, rr), public) and engine.torch.equal(probe.gc_x_mod_n_equals(N, rx, fin, rr), public)
