#!/usr/bin/env python3
"""Host model of Ed25519 batch verification as ecsimd_ed25519_verify_batch does it (include/ecsimd_ed25519_batch.h), on Python integers, `hashlib` and
ed25519_model only: the NORMATIVE statement of the cofactored per-lane rule, of the randomizers and of the batch verdict.

The per-lane rule (verify_cofactored): s < L; A AND R decode strictly (y < p, a root exists, not x = 0 with the sign bit set); and
[8]([s]B - [h]A - R) is the identity, h = SHA-512(R || A || M) mod L over the bytes as given.  Strict encodings with the cofactored equation: NOT ZIP-215,
which also accepts non-canonical encodings.  reject_small_order refuses the eight small-order encodings as A or R as well.

A batch of n signatures (A_i, M_i, R_i || s_i); s_i enters the hashes as its 32 bytes as given:

    D_i    = SHA-512(R_i || A_i || M_i)                                           all 64 bytes; h_i = int(D_i, little-endian) mod L
    leaf_i = H_"ecsimd/ed25519-batch/leaf"(D_i || s_i)                            D_i binds R, A and the message: the message is hashed once
    node   = H_"ecsimd/ed25519-batch/node"(c_0 || ... || c_{k-1})                 k <= 16 children in lane order; levels until one digest remains
    seed   = H_"ecsimd/ed25519-batch/seed"(root || n as 8 big-endian bytes)       n = 1: root = leaf_0
    z_i    = (int(H_"ecsimd/ed25519-batch/a"(seed || i as 8 big-endian bytes), big-endian) mod 2^128) | 1

H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x), the tagged hash tools/schnorr_batch_model.py uses.  A malformed lane (s >= L, A or R does not decode, or
small-order with the flag) refuses the batch; otherwise the batch is accepted iff

    [8]( sum z_i R_i  +  [ sum (z_i h_i mod L) A_i + (L - sum z_i s_i mod L) B ] )  =  the identity.

DETERMINISM: reducing z_i h_i modulo L changes the term by a multiple of [L]A_i, a torsion point, which the 8 kills: the verdict is a function of the batch.
SOUNDNESS: for a lane that fails the per-lane rule the prime-order part of [s]B - [h]A - R is not the identity, so the prime-order part of the sum is a nonzero
linear form in the z_i over a group of prime order: it vanishes for at most 2^-127 of the seeds, and the seed is a hash of the batch.
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ed25519_model as ed  # noqa: E402

TAG_LEAF, TAG_NODE, TAG_SEED, TAG_A = (
    "ecsimd/ed25519-batch/leaf", "ecsimd/ed25519-batch/node", "ecsimd/ed25519-batch/seed", "ecsimd/ed25519-batch/a")
# the midstates k_msm_ed25519.hip holds as literals, in its order
DEVICE_TAGS = (TAG_LEAF, TAG_NODE, TAG_SEED, TAG_A)
FAN = 16
L, P = ed.L, ed.P


def tagged_hash(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


_SHA256_K = None


def midstate(tag):
    """The eight words of the SHA-256 state after the block SHA256(tag) || SHA256(tag) (hashlib does not expose it: FIPS 180-4 restated)."""
    global _SHA256_K
    if _SHA256_K is None:
        primes, v = [], 2
        while len(primes) < 64:
            if all(v % q for q in primes):
                primes.append(v)
            v += 1

        def frac_root(p, k):               # the first 32 bits of the fractional part of p^(1/k), exactly
            lo, hi = 0, 1 << 40
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if mid ** k <= p << (32 * k):
                    lo = mid
                else:
                    hi = mid
            return lo & 0xffffffff
        _SHA256_K = ([frac_root(p, 3) for p in primes], [frac_root(p, 2) for p in primes[:8]])
    K, iv = _SHA256_K
    t = hashlib.sha256(tag.encode()).digest()
    block = t + t
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & 0xffffffff
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & 0xffffffff)
    a, b, c, d, e, f, g, h = iv
    for i in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i]) & 0xffffffff
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xffffffff
        a, b, c, d, e, f, g, h = (t1 + t2) & 0xffffffff, a, b, c, (d + t1) & 0xffffffff, e, f, g
    return [(x + y) & 0xffffffff for x, y in zip(iv, (a, b, c, d, e, f, g, h))]


# ---- the per-lane rule
def digest(pk, msg, sig):
    return hashlib.sha512(sig[:32] + pk + msg).digest()


def malformed(pk, sig, reject_small_order=False):
    """s >= L, A or R does not decode, or (with the flag) a small-order encoding."""
    if len(pk) != 32 or len(sig) != 64 or int.from_bytes(sig[32:], "little") >= L:
        return True
    if ed.decode(pk) is None or ed.decode(sig[:32]) is None:
        return True
    return bool(reject_small_order and (pk in ed.SMALL_ORDER or sig[:32] in ed.SMALL_ORDER))


def times8(p):
    return ed.pt_dbl(ed.pt_dbl(ed.pt_dbl(p)))


def verify_cofactored(pk, msg, sig, reject_small_order=False):
    if malformed(pk, sig, reject_small_order):
        return False
    a, r, s = ed.decode(pk), ed.decode(sig[:32]), int.from_bytes(sig[32:], "little")
    h = int.from_bytes(digest(pk, msg, sig), "little") % L
    defect = ed.pt_add(ed.pt_add(ed.base_point_mul(s), ed.pt_mul(h, ed.pt_neg(a))), ed.pt_neg(r))
    return ed.pt_eq(times8(defect), ed.IDENTITY)


# ---- the randomizers
def leaf(pk, msg, sig):
    return tagged_hash(TAG_LEAF, digest(pk, msg, sig) + sig[32:])


def root(leaves):
    level = list(leaves)
    assert level
    while len(level) > 1:
        level = [tagged_hash(TAG_NODE, b"".join(level[i:i + FAN])) for i in range(0, len(level), FAN)]
    return level[0]


def seed(leaves):
    return tagged_hash(TAG_SEED, root(leaves) + len(leaves).to_bytes(8, "big"))


def randomizers(pks, msgs, sigs):
    """z_0 .. z_{n-1} for the batch; malformed lanes included (their bytes are hashed as they are).  Messages may differ in length."""
    n = len(pks)
    assert len(msgs) == len(sigs) == n
    if n == 0:
        return []
    sd = seed([leaf(pk, m, sg) for pk, m, sg in zip(pks, msgs, sigs)])
    return [(int.from_bytes(tagged_hash(TAG_A, sd + i.to_bytes(8, "big")), "big") % (1 << 128)) | 1 for i in range(n)]


# ---- the sums
def msm(scalars, points):
    """The exact integer combination sum k_i P_i of extended points (scalars are integers, not residues: the points may carry torsion)."""
    acc = ed.IDENTITY
    for k, p in zip(scalars, points):
        acc = ed.pt_add(acc, ed.pt_mul(k, p))
    return acc


def msm_encoded(scalars, encodings, bits=256):
    """(encoding of sum (k_i mod 2^bits) P_i over the encodings that decode, finite, invalid) as ecsimd_ed25519_msm reports it."""
    pts = [ed.decode(e) for e in encodings]
    acc = msm([k % (1 << bits) for k, p in zip(scalars, pts) if p is not None], [p for p in pts if p is not None])
    return ed.encode(acc), int(not ed.pt_eq(acc, ed.IDENTITY)), sum(1 for p in pts if p is None)


def batch_verify(pks, msgs, sigs, reject_small_order=False, z=None):
    """The verdict of the MSM route.  `z`: other randomizers than the model's (a test passes all ones to show what the weights are for)."""
    z = randomizers(pks, msgs, sigs) if z is None else z
    if any(malformed(pk, sg, reject_small_order) for pk, sg in zip(pks, sigs)):
        return False
    sum_r, sum_a, s_sum = ed.IDENTITY, ed.IDENTITY, 0
    for zi, pk, m, sg in zip(z, pks, msgs, sigs):
        h = int.from_bytes(digest(pk, m, sg), "little") % L
        sum_r = ed.pt_add(sum_r, ed.pt_mul(zi, ed.decode(sg[:32])))
        sum_a = ed.pt_add(sum_a, ed.pt_mul(zi * h % L, ed.decode(pk)))
        s_sum = (s_sum + zi * int.from_bytes(sg[32:], "little")) % L
    sum_a = ed.pt_add(sum_a, ed.base_point_mul((L - s_sum) % L))
    return ed.pt_eq(times8(ed.pt_add(sum_r, sum_a)), ed.IDENTITY)


def batch_verify_lanes(pks, msgs, sigs, reject_small_order=False):
    """The verdict of the LANES route: the AND of the per-lane rule; 1 for an empty batch."""
    return all(verify_cofactored(pk, m, sg, reject_small_order) for pk, m, sg in zip(pks, msgs, sigs))


if __name__ == "__main__":
    for tag in DEVICE_TAGS:
        print("      {" + ", ".join("0x%08xu" % w for w in midstate(tag)) + "},   // " + tag)
