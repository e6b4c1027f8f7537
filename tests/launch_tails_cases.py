"""The input batches of tests/test_gpu_launch_tails.py, as Python integers, and the choice of the surrogate orders -- shared with tests/test_launch_tails_cpu.py,
which checks on the CPU what the GPU test asserts of every batch before it looks at the device's answer.  Expected values are NOT made here: they come from
tools/launch_tails_model.py in the tests.  A batch is a function of its name and of the order alone (the random lanes do not change with the order: only the
lanes placed AT the order, beside it, or at n' - IL do).

A plain module, not a conftest: nothing here is collected.
"""
import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import launch_tails_model as model  # noqa: E402

LANES = 300                      # one workgroup of 256 and a partial one
N, P, HARDENED = model.N, model.P, model.HARDENED
# A surrogate order: odd, between 2^255 and 3 * 2^254, so that between a quarter and a half of uniformly random digests are at or above it.
HALF = 0xa5b1c3d7e9f20416283a4c5e70819335577991b3d5f7092b4d6f8193a5c7e9fb
assert HALF & 1 and 1 << 255 < HALF < 3 << 254
MIN_SIDE = 64                    # lanes of a batch that must fall on each side of HALF
ZERO_BLOCK = range(200, 230)     # triples of lanes: the key that makes the sum 0, and its two neighbours
# (bytes, row stride, first column).  sha256_absorb_message looks at the alignment only where a whole 64-byte block fits, so 32 bytes (contiguous words) and 45
# bytes (odd stride and start) go through the padded tail alone, and 77 bytes come twice: a whole block by word loads, and by byte loads.
MSG_SHAPES = ((32, 32, 0), (45, 47, 1), (77, 80, 0), (77, 79, 1))
SEED_BYTES = (16, 33, 64)


def _rng(name):
    return random.Random("launch tails / " + name)


def _r256(rng):
    return rng.getrandbits(256)


def _low(rng):
    return rng.getrandbits(255) | 1          # in [1, 2^255): inside every order


def _liftable(rng, want=True):
    while True:
        x = rng.randrange(P)
        if (model.lift_even(x) is not None) == want:
            return x


def _curve_point(rng):
    x, y = model.lift_even(_liftable(rng))
    return (x, P - y) if rng.getrandbits(1) else (x, y)


@functools.lru_cache(maxsize=None)         # (the same for every order)
def messages(name, shape):
    """LANES messages of shape[0] bytes and the whole byte array they are a column slice of (rows of shape[1] bytes, the messages from column shape[2])."""
    nbytes, stride, first = shape
    rng = _rng(f"messages {name} {shape}")
    rows = [rng.randbytes(stride) for _ in range(LANES)]
    return [row[first:first + nbytes] for row in rows], rows


# ---- the batches.  Every builder returns a dict of lists of LANES values, `digest` = the hash each lane's kernel compares with the order, and `free` = the
# lanes whose digest and standing do not depend on the order (where a fitted order may be placed).
def master(seed_bytes):
    rng = _rng(f"master {seed_bytes}")
    seeds = [rng.randbytes(seed_bytes) for _ in range(LANES)]
    return dict(seed=seeds, digest=[model.master_digest(s)[0] for s in seeds], free=list(range(LANES)))


def ckd_priv(n, with_point):
    rng = _rng(f"ckd_priv {with_point}")
    k, c, index, pt = [], [], [], []
    for i in range(LANES):
        k.append(_low(rng) if i % 2 == 0 else _r256(rng))
        c.append(_r256(rng))
        index.append(rng.getrandbits(31) | (HARDENED if rng.getrandbits(1) else 0))
        pt.append((_r256(rng), _r256(rng)))          # the kernel hashes the arrays as given: any 256-bit values will do, of either parity
    for i, v in enumerate((0, n, n - 1, 1, 0, n, n - 1, 1)):
        k[i] = v
        index[i] = (index[i] & (HARDENED - 1)) | (HARDENED if i < 4 else 0)
    if with_point:                                   # not hardened, so IL does not depend on k_par: k_par = n - IL makes the child key 0
        for i in ZERO_BLOCK:
            index[i] &= HARDENED - 1
            il = model.ckd_priv_digest(0, c[i], index[i], pt[i])[0]
            k[i] = (n - il + (0, 1, -1)[(i - ZERO_BLOCK.start) % 3]) % n
    point = pt if with_point else [None] * LANES
    digest = [model.ckd_priv_digest(k[i], c[i], index[i], point[i])[0] for i in range(LANES)]
    free = [i for i in range(8, ZERO_BLOCK.start, 2) if with_point or index[i] >= HARDENED]
    return dict(k=k, c=c, index=index, point=point, digest=digest, free=free)


def ckd_pub_front():
    rng = _rng("ckd_pub_front")
    qx, qy, c, index, free = [], [], [], [], []
    for i in range(LANES):
        x, y = _curve_point(rng)
        idx = rng.getrandbits(31)
        if i % 5 == 3:
            y = (y + 1 + rng.getrandbits(1)) % P     # off the curve (y + 1 keeps the parity bit's flip, y + 2 the parity)
        elif i % 5 == 4:
            idx |= HARDENED
        elif i % 10 == 7:
            idx |= HARDENED; y ^= 2                  # both causes at once
        else:
            free.append(i)
        qx.append(x); qy.append(y); c.append(_r256(rng)); index.append(idx)
    qx[0], qy[1] = P, P + 1                          # a coordinate that is not below p
    qx[2], qy[2] = (1 << 256) - 1, (1 << 256) - 1
    free = [i for i in free if i > 2]
    digest = [model.ckd_pub_digest(qx[i], qy[i], c[i], index[i])[0] for i in range(LANES)]
    return dict(qx=qx, qy=qy, c=c, index=index, digest=digest, free=free)


def ckd_pub_accept():
    rng = _rng("ckd_pub_accept")
    jzs = (0, 1, 1 << 255, 1 << 64, None, None)
    valids = (0, 1, 0, 1, 2, 255, 0, 1)
    return dict(ax=[_r256(rng) for _ in range(LANES)], ay=[_r256(rng) for _ in range(LANES)], c=[_r256(rng) | 1 for _ in range(LANES)],
                jz=[(lambda v: _r256(rng) | 1 if v is None else v)(jzs[i % 6]) for i in range(LANES)], valid=[valids[(i // 6) % 8] for i in range(LANES)])


def verify_front(n, shape):
    rng = _rng("verify_front")
    msgs, rows = messages("verify_front", shape)
    px, r, s, free = [], [], [], []
    for i in range(LANES):
        px.append(_liftable(rng, want=i % 7 != 5))
        r.append(rng.randrange(P))
        s.append(_low(rng) if i % 2 == 0 else _r256(rng))
        if i % 7 != 5 and i % 2 == 0 and i >= 8:
            free.append(i)
    s[0], s[1], s[6] = n - 1, n, (1 << 256) - 1
    r[2], r[3], r[7] = P - 1, P, (1 << 256) - 1
    px[4] = P
    digest = [model.challenge_digest(r[i], px[i], msgs[i]) for i in range(LANES)]
    return dict(px=px, r=r, s=s, msgs=msgs, rows=rows, digest=digest, free=free)


def nonce(n, shape, with_aux):
    rng = _rng("nonce")
    msgs, rows = messages("nonce", shape)
    d = [_low(rng) if i % 2 == 0 else _r256(rng) for i in range(LANES)]
    d[0], d[1], d[2], d[3] = 0, n, n - 1, 1
    aux = [_r256(rng) for _ in range(LANES)] if with_aux else [None] * LANES
    px, py = [_r256(rng) for _ in range(LANES)], [_r256(rng) for _ in range(LANES)]
    digest = [model.nonce_digest(n, d[i], aux[i], px[i], py[i], msgs[i]) for i in range(LANES)]
    free = [i for i in range(4, LANES, 2) if py[i] & 1 == 0]          # d' = d: the hash does not depend on the order
    return dict(d=d, aux=aux, px=px, py=py, msgs=msgs, rows=rows, digest=digest, free=free)


def finish(n, shape):
    rng = _rng("finish")
    msgs, rows = messages("finish", shape)
    d = [1 + rng.randrange(n - 1) for _ in range(LANES)]
    k0 = [1 + rng.randrange(n - 1) for _ in range(LANES)]
    for i in range(0, LANES, 10):                    # refused by the nonce kernel: k0 = 0, and d may be anything
        k0[i], d[i] = 0, (0, n, _r256(rng))[(i // 10) % 3]
    k0[1], k0[2], d[3], d[4] = n - 1, 1, n - 1, 1
    xP, yP, xR, yR = ([_r256(rng) for _ in range(LANES)] for _ in range(4))
    digest = [model.challenge_digest(xR[i], xP[i], msgs[i]) for i in range(LANES)]
    return dict(d=d, k0=k0, xP=xP, yP=yP, xR=xR, yR=yR, msgs=msgs, rows=rows, digest=digest, free=[])


def tweak_front(has_root):
    rng = _rng(f"tweak_front {has_root}")
    px = [_liftable(rng, want=i % 7 != 5) for i in range(LANES)]
    px[0], px[1] = P, (1 << 256) - 1
    merkle = [_r256(rng) if has_root else None for _ in range(LANES)]
    digest = [model.tap_tweak(px[i], merkle[i]) for i in range(LANES)]
    return dict(px=px, merkle=merkle, digest=digest, free=[i for i in range(2, LANES) if i % 7 != 5])


def taproot_seckey(n, has_root):
    rng = _rng(f"taproot_seckey {has_root}")
    d = [_low(rng) if i % 2 == 0 else _r256(rng) for i in range(LANES)]
    d[0], d[1], d[2], d[3] = 0, n, n - 1, 1
    xP, yP = [_r256(rng) for _ in range(LANES)], [_r256(rng) for _ in range(LANES)]
    merkle = [_r256(rng) if has_root else None for _ in range(LANES)]
    digest = [model.tap_tweak(xP[i], merkle[i]) for i in range(LANES)]
    for i in ZERO_BLOCK:                             # d' = n - t makes the sum 0; d = d' or n - d' by the parity the kernel will see
        dd = (n - digest[i] + (0, 1, -1)[(i - ZERO_BLOCK.start) % 3]) % n
        d[i] = (n - dd) % n if yP[i] & 1 else dd
    return dict(d=d, xP=xP, yP=yP, merkle=merkle, digest=digest, free=list(range(4, ZERO_BLOCK.start, 2)))


def recovery_id():
    rng = _rng("recovery_id")
    x, y, s, ok = [], [], [], []
    for i in range(LANES):
        x.append((N - 1, N, N + 1, P - 1, rng.randrange(N), N + rng.randrange(P - N))[i % 6])
        y.append((rng.randrange(P) & ~1) | ((i // 6) & 1))
        s.append((1, (N - 1) // 2, (N + 1) // 2, N - 1, 1 + rng.randrange(N - 1), 1 + rng.randrange(N - 1))[(i // 12) % 6])
        ok.append(0 if i % 25 == 24 else 1)
        if not ok[i]:
            s[i] = 0                                 # what ecdsa_sign_scalars leaves in a refused lane
    return dict(x=x, y=y, s=s, ok=ok)


def sign_scalars():
    rng = _rng("sign_scalars")
    e = [_r256(rng) for _ in range(LANES)]
    d = [1 + rng.randrange(N - 1) for _ in range(LANES)]
    k = [1 + rng.randrange(N - 1) for _ in range(LANES)]
    x = [rng.randrange(P) for _ in range(LANES)]
    for i in range(LANES):
        if i % 5 == 1:
            x[i] = N + rng.randrange(P - N)          # r = x - n
        elif i % 5 == 2 and i < 100:
            x[i] = N                                 # r = 0
    for i in range(100, 160):                        # triples: s = 0 at d = -e / r, served at its neighbours
        r = x[i] % N
        d[i] = (-e[i] * pow(r, -1, N) + (0, 1, -1)[(i - 100) % 3]) % N
    d[0], d[5], k[10], k[15], e[20], e[25] = 0, N, 0, N, 0, N
    return dict(e=e, d=d, k=k, x=x)


def x_mod_n():
    rng = _rng("x_mod_n")
    x, r, finite = [], [], []
    for i in range(LANES):
        small = rng.randrange(P - N)                 # r + n < p only for such an r
        big = rng.randrange(N)
        xi, ri = ((big, big), (small + N, small), (small + N, (small + 1) % N), (big, (big + 1) % N), (small + N, small + N), (N, 0), (small, small), (N - 1, N - 1))[i % 8]
        x.append(xi); r.append(ri); finite.append(0 if (i // 8) % 4 == 3 else (1, 2, 255)[i % 3])
    return dict(x=x, r=r, finite=finite)


# Every batch that is compared with an order: name -> builder(n)
BATCHES = {}
for _length in SEED_BYTES:
    BATCHES[f"master {_length}"] = lambda n, _l=_length: master(_l)
for _flag in (True, False):
    BATCHES[f"ckd_priv {_flag}"] = lambda n, _f=_flag: ckd_priv(n, _f)
    BATCHES[f"tweak_front {_flag}"] = lambda n, _f=_flag: tweak_front(_f)
    BATCHES[f"taproot_seckey {_flag}"] = lambda n, _f=_flag: taproot_seckey(n, _f)
BATCHES["ckd_pub_front"] = lambda n: ckd_pub_front()
for _shape in MSG_SHAPES:
    BATCHES[f"verify_front {_shape[0]}+{_shape[2]}"] = lambda n, _s=_shape: verify_front(n, _s)
    BATCHES[f"nonce {_shape[0]}+{_shape[2]}"] = lambda n, _s=_shape: nonce(n, _s, with_aux=_s[0] != 32)
    BATCHES[f"finish {_shape[0]}+{_shape[2]}"] = lambda n, _s=_shape: finish(n, _s)


# ---- the orders
def sides(digest, n):
    """(lanes whose digest is below n, lanes at or above it)"""
    below = sum(1 for h in digest if h < n)
    return below, len(digest) - below


def fitted_orders(batch):
    """[(n', lane, where)]: four orders that put one free lane's digest H at n' exactly, at n' - 2, at n' - 1 and at n' + 1.  H is above 2^255 and of the
    parity that makes n' odd, so n' is an order the kernels can take."""
    top = 1 << 255
    odd = next(i for i in batch["free"] if batch["digest"][i] > top and batch["digest"][i] & 1)
    even = next(i for i in batch["free"] if batch["digest"][i] > top + 2 and not batch["digest"][i] & 1)
    h, g = batch["digest"][odd], batch["digest"][even]
    out = [(h, odd, 0), (h + 2, odd, -2), (g + 1, even, -1), (g - 1, even, 1)]
    for n, _, _ in out:
        model.check_order(n)
    return out


def assert_placed(batch, n, lane, where):
    """What the test says of a fitted order, from the model's digest alone: the lane sits at n + where, and the order-independent lanes are where they were."""
    assert lane in batch["free"] and batch["digest"][lane] == n + where, (lane, where)
