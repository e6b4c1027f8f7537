#!/usr/bin/env python3
"""Host model of BIP-340 batch verification as ecsimd_schnorr_verify_batch does it (include/ecsimd_schnorr_batch.h), on Python integers, `hashlib` and
bip340_model only: the NORMATIVE statement of the randomizers and of the verdict.

A batch of u signatures (px_i, m_i, r_i, s_i), all messages of one length; integers are the big-endian reading of their 32 bytes, b(x) below.

    E_i    = H_"BIP0340/challenge"(b(r_i) || b(px_i) || m_i)                       the full 32-byte digest; e_i = int(E_i) mod n
    leaf_i = H_"ecsimd/schnorr-batch/leaf"(E_i || b(s_i))                          E_i binds r, px and the message: the message is hashed once
    node   = H_"ecsimd/schnorr-batch/node"(c_0 || ... || c_{k-1})                  k <= 16 children in lane order; levels until one digest remains
    seed   = H_"ecsimd/schnorr-batch/seed"(root || u as 8 big-endian bytes)        u = 1: root = leaf_0
    a_i    = (int(H_"ecsimd/schnorr-batch/a"(seed || i as 8 big-endian bytes)) mod 2^128) | 1

H_tag(x) = SHA256(SHA256(tag) || SHA256(tag) || x), BIP-340's tagged hash.  Every a_i is odd and below 2^128, and every a_i depends on every byte of the batch
and on i.  The batch is accepted iff every lane is well formed (px and r lift to points P_i, R_i with even y; s_i < n) and

    sum a_i R_i  +  sum (a_i e_i mod n) P_i  +  (n - sum a_i s_i mod n) G  =  the point at infinity.

A valid batch always passes.  If some lane is not a valid signature the left side is a nonzero linear form in the a_i over a group of prime order, and a_i takes
2^127 values: the batch passes with probability at most 2^-127 over the seed -- and whoever chooses the signatures cannot choose the seed, it is a hash of them.
"""
import bip340_model as b340

TAG_LEAF, TAG_NODE, TAG_SEED, TAG_A = (
    "ecsimd/schnorr-batch/leaf", "ecsimd/schnorr-batch/node", "ecsimd/schnorr-batch/seed", "ecsimd/schnorr-batch/a")
# the midstates k_schnorr_batch.hip holds as literals, in its order (the last one is BIP-340's own challenge tag)
DEVICE_TAGS = (TAG_LEAF, TAG_NODE, TAG_SEED, TAG_A, "BIP0340/challenge")
FAN = 16
N, P = b340.N, b340.P


def _b(x):
    return x.to_bytes(32, "big")


def challenge_digest(px, msg, r):
    return b340.tagged_hash("BIP0340/challenge", _b(r) + _b(px) + msg)


def leaf(px, msg, r, s):
    return b340.tagged_hash(TAG_LEAF, challenge_digest(px, msg, r) + _b(s))


def root(leaves):
    level = list(leaves)
    assert level
    while len(level) > 1:
        level = [b340.tagged_hash(TAG_NODE, b"".join(level[i:i + FAN])) for i in range(0, len(level), FAN)]
    return level[0]


def seed(leaves):
    return b340.tagged_hash(TAG_SEED, root(leaves) + len(leaves).to_bytes(8, "big"))


def randomizers(pxs, msgs, rs, ss):
    """a_0 .. a_{u-1} for the batch; integers below 2^256 in, malformed lanes included (their bytes are hashed as they are)."""
    u = len(pxs)
    assert len(msgs) == len(rs) == len(ss) == u and len({len(m) for m in msgs}) <= 1
    if u == 0:
        return []
    sd = seed([leaf(px, m, r, s) for px, m, r, s in zip(pxs, msgs, rs, ss)])
    return [(int.from_bytes(b340.tagged_hash(TAG_A, sd + i.to_bytes(8, "big")), "big") % (1 << 128)) | 1 for i in range(u)]


def batch_verify(pxs, msgs, rs, ss, a=None):
    """The verdict.  `a`: other randomizers than the model's (a test passes all ones to show what the weights are for)."""
    u = len(pxs)
    a = randomizers(pxs, msgs, rs, ss) if a is None else a
    acc, s_sum = None, 0
    for ai, px, m, r, s in zip(a, pxs, msgs, rs, ss):
        Pi, Ri = b340.lift_x(px) if px < (1 << 256) else None, b340.lift_x(r) if r < (1 << 256) else None
        if Pi is None or Ri is None or s >= N:
            return False
        e = int.from_bytes(challenge_digest(px, m, r), "big") % N
        acc = b340.add(acc, b340.mul(ai, Ri))
        acc = b340.add(acc, b340.mul(ai * e % N, Pi))
        s_sum = (s_sum + ai * s) % N
    acc = b340.add(acc, b340.mul_g((N - s_sum) % N))
    return acc is None


if __name__ == "__main__":
    for tag in DEVICE_TAGS:
        print("      {" + ", ".join("0x%08xu" % w for w in b340.midstate(tag)) + "},   // " + tag)
