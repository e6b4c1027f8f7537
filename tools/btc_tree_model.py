#!/usr/bin/env python3
"""Host model of the two trees Bitcoin builds of SHA-256: a block's Merkle tree with Bitcoin Core's `mutated` flag, and BIP-341's script tree -- compact
sizes, TapLeaf hashes, the TapBranch walk up a control block's path, a small taptree builder that yields every leaf's path, and the script-path check.

What ecsimd_hip_btc_merkle_root, _tapleaf_hash and _taproot_merkle_path promise, written down once without any of the library's code: hashlib, and the
tagged hash, the midstate and the key tweak of tools/btc_model.py.  tests/test_btc_tree_cpu.py pins this model to tests/golden/btc_tree_vectors.json (block
170's Merkle root and BIP-341's wallet vector with one script); `python tools/btc_tree_model.py --mint` writes that file's midstates.

Bytes in and out: a txid, a leaf hash and a node are the 32 digest bytes in hashing order (a txid as explorers print it is those bytes reversed).
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from btc_model import midstate, sha256d, tagged_hash, taproot_tweak_pubkey   # noqa: E402


# ---- Merkle roots (Bitcoin Core, consensus/merkle.cpp: ComputeMerkleRoot)
def merkle_root(leaves):
    """(root, mutated) of a non-empty list of 32-byte leaves.  mutated: some level holds a REAL pair (both nodes exist) of two equal values -- the sign of
    CVE-2012-2459's duplicated transactions; it is looked for before the level's last node is paired with itself."""
    assert leaves and all(len(x) == 32 for x in leaves)
    level, mutated = list(leaves), False
    while len(level) > 1:
        mutated = mutated or any(level[j] == level[j + 1] for j in range(0, len(level) - 1, 2))
        if len(level) & 1:
            level.append(level[-1])
        level = [sha256d(level[j] + level[j + 1]) for j in range(0, len(level), 2)]
    return level[0], mutated


# ---- BIP-341 script trees
def compact_size(n):
    """Bitcoin's variable-length integer, as far as a script's length goes (below 2^32)."""
    assert 0 <= n < 2**32
    if n < 0xfd:
        return bytes([n])
    if n <= 0xffff:
        return b"\xfd" + n.to_bytes(2, "little")
    return b"\xfe" + n.to_bytes(4, "little")


def tapleaf_hash(script, leaf_version=0xc0):
    return tagged_hash("TapLeaf", bytes([leaf_version]) + compact_size(len(script)) + script)


def tapbranch_hash(a, b):
    return tagged_hash("TapBranch", min(a, b) + max(a, b))


def merkle_path_root(leaf, path):
    """The root a leaf hash reaches over the nodes of a control block's path (a list of 32-byte values, the leaf's sibling first); None beyond BIP-341's depth of 128."""
    if len(path) > 128:
        return None
    k = leaf
    for e in path:
        k = tapbranch_hash(k, e)
    return k


def taptree(tree):
    """(root, [(script, leaf_version, path), ...]) of a tree given as nested pairs whose leaves are (script, leaf_version) tuples of bytes and int -- a single
    leaf is a tree.  The leaves come in depth-first order, each with the path its control block holds."""
    if isinstance(tree[0], (bytes, bytearray)):
        script, version = tree
        return tapleaf_hash(script, version), [(script, version, [])]
    (lh, left), (rh, right) = taptree(tree[0]), taptree(tree[1])
    return tapbranch_hash(lh, rh), [(s, v, p + [rh]) for s, v, p in left] + [(s, v, p + [lh]) for s, v, p in right]


def control_block(internal_key, output_parity, leaf_version, path):
    return bytes([leaf_version | output_parity]) + internal_key.to_bytes(32, "big") + b"".join(path)


def script_path_ok(output_key, control, script):
    """BIP-341's script-path check of one input: the control block (33 + 32 d bytes, d <= 128) and the script commit to the x-only output key (an integer)."""
    if len(control) < 33 or (len(control) - 33) % 32 or (len(control) - 33) // 32 > 128:
        return False
    px = int.from_bytes(control[1:33], "big")
    path = [control[33 + 32 * j:65 + 32 * j] for j in range((len(control) - 33) // 32)]
    root = merkle_path_root(tapleaf_hash(script, control[0] & 0xfe), path)
    q = taproot_tweak_pubkey(px, int.from_bytes(root, "big"))
    return q is not None and q == (output_key, control[0] & 1)


def mint(path):
    """Fills in the fixture's midstates (the state after each tag block, by the plain-Python compression function); the published values stay as they are."""
    doc = json.load(open(path))
    doc["tapleaf_midstate"] = ["%08x" % x for x in midstate("TapLeaf")]
    doc["tapbranch_midstate"] = ["%08x" % x for x in midstate("TapBranch")]
    json.dump(doc, open(path, "w"), indent=1)
    open(path, "a").write("\n")


if __name__ == "__main__":
    fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "btc_tree_vectors.json")
    if "--mint" in sys.argv:
        mint(fixture)
    a, b, c = (hashlib.sha256(bytes([i])).digest() for i in range(3))
    for leaves in ([a], [a, b, c], [a, b, c, c]):
        root, mutated = merkle_root(leaves)
        print(len(leaves), root.hex(), int(mutated))
