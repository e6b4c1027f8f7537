"""GPU suite: Bitcoin's hashes with one length per lane, Merkle roots, and BIP-341 script paths (k_btc_tree.hip).

Every expectation comes from hashlib, tools/btc_model.py or tools/btc_tree_model.py (pinned to published values by tests/test_btc_tree_cpu.py) -- never from
the call under test.  Every lane of every batch is compared.
"""
import functools
import hashlib
import json
import os
import random
import sys

import numpy as np
import pytest

from helpers import ints_to_arr, arr_to_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import btc_model        # noqa: E402
import btc_tree_model as model  # noqa: E402

pytestmark = pytest.mark.gpu
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "btc_tree_vectors.json")))
HASHES = {"sha256": lambda m: hashlib.sha256(m).digest(), "sha256d": btc_model.sha256d, "hash160": btc_model.hash160, "ripemd160": btc_model.ripemd160}
CYCLE = [0, 1, 3, 4, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 200]
LANES, STRIDE = 3 * 64 + 5, 200


def up(engine, ints):
    return engine.to_device(ints_to_arr([int(x) for x in ints]))


def up32(engine, digests):
    return up(engine, [int.from_bytes(d, "big") for d in digests])


def digests32(engine, e):
    return [v.to_bytes(32, "big") for v in arr_to_ints(engine.to_numpy(e))]


def flags(t):
    return [int(v) for v in t.cpu().numpy()]


def rows(engine, host, stride, offset, n, length):
    """`host` (bytes of n records `stride` apart) on the device `offset` bytes behind a 16-byte aligned base, as the (n, length) strided view the engine takes."""
    import torch
    raw = torch.zeros(offset + n * stride + 16, dtype=torch.uint8, device=engine.tdev)
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + len(host)] = torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(engine.tdev)
    return raw.as_strided((n, length), (stride, 1), offset)


def lens_of(engine, lens):
    import torch
    return torch.tensor(lens, dtype=torch.int32, device=engine.tdev)


def bytes_of(engine, values):
    import torch
    return torch.tensor(values, dtype=torch.uint8, device=engine.tdev)


def run_hash(engine, name, view, lens):
    out = getattr(engine, name)(view, None if lens is None else lens_of(engine, lens))
    return digests32(engine, out) if name.startswith("sha256") else [bytes(r) for r in out.cpu().numpy()]


def filled(messages, stride, fill):
    return b"".join(m + bytes([fill]) * (stride - len(m)) for m in messages)


# ---- 1. one length per lane
@functools.lru_cache(maxsize=None)
def mixed_messages():
    rng = random.Random(1)
    return [rng.randbytes(CYCLE[i % len(CYCLE)]) for i in range(LANES)]


@functools.lru_cache(maxsize=None)
def mixed_expected(name):
    return [HASHES[name](m) for m in mixed_messages()]


@pytest.mark.parametrize("offset", [0, 4, 1, 3])
@pytest.mark.parametrize("name", sorted(HASHES))
def test_every_lane_hashes_its_own_length(engine, name, offset):
    """3 x 64 + 5 lanes whose lengths cycle through the shapes of the padding, so every wave mixes trip counts; a base that is a multiple of 4 takes word loads,
    an odd one byte loads.  What lies behind a lane's message reaches no digest."""
    msgs = mixed_messages()
    lens = [len(m) for m in msgs]
    got = run_hash(engine, name, rows(engine, filled(msgs, STRIDE, 0xA5), STRIDE, offset, LANES, STRIDE), lens)
    assert got == mixed_expected(name)
    assert run_hash(engine, name, rows(engine, filled(msgs, STRIDE, 0x3C), STRIDE, offset, LANES, STRIDE), lens) == got


@pytest.mark.parametrize("name", sorted(HASHES))
def test_a_length_above_the_stride_is_the_stride_and_equal_lengths_are_the_equal_length_call(engine, name):
    rng = random.Random(2)
    n, stride = 70, 132
    host = rng.randbytes(n * stride)
    view = rows(engine, host, stride, 0, n, stride)
    expected = [HASHES[name](host[i * stride:(i + 1) * stride]) for i in range(n)]
    assert run_hash(engine, name, view, [stride + 1 + 1000 * i for i in range(n)]) == expected
    for length in (128, 55, 0):
        same = run_hash(engine, name, view, [length] * n)
        assert same == run_hash(engine, name, view[:, :length], None) == [HASHES[name](host[i * stride:i * stride + length]) for i in range(n)]


@pytest.mark.parametrize("name", sorted(HASHES))
def test_one_long_message_among_short_ones(engine, name):
    rng = random.Random(3)
    n, stride = 70, 65536
    msgs = [rng.randbytes(rng.randrange(0, 90)) for _ in range(n)]
    msgs[37] = rng.randbytes(65536)
    got = run_hash(engine, name, rows(engine, filled(msgs, stride, 0xA5), stride, 0, n, stride), [len(m) for m in msgs])
    assert got == [HASHES[name](m) for m in msgs]


# ---- 2. Merkle roots
def random_trees(rng, counts):
    return [[rng.randbytes(32) for _ in range(c)] for c in counts]


def check_trees(engine, trees):
    leaves = up32(engine, [x for t in trees for x in t])
    return leaves, [len(t) for t in trees], [model.merkle_root(t) for t in trees]


def assert_roots(engine, got, expected):
    roots, mutated = got
    assert digests32(engine, roots) == [r for r, _ in expected]
    assert flags(mutated) == [int(m) for _, m in expected]


def test_merkle_roots_of_trees_of_every_shape(engine):
    trees = random_trees(random.Random(4), [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 255, 257, 4097])
    leaves, counts, expected = check_trees(engine, trees)
    assert_roots(engine, engine.btc_merkle_root(leaves, counts, want_mutated=True), expected)
    assert digests32(engine, engine.btc_merkle_root(leaves, counts)) == [r for r, _ in expected]            # mutated = NULL


def test_many_small_trees_and_two_calls_back_to_back(engine):
    """300 trees: the lane -> tree lookup crosses thread blocks.  A second call of another shape follows the first without a synchronisation, then the first one
    again: the levels in the workspace and the staged offsets of one call are not the next one's."""
    rng = random.Random(5)
    small = random_trees(rng, [rng.randrange(1, 41) for _ in range(300)])
    other = random_trees(rng, [700, 1, 2, 65])
    a, ca, ea = check_trees(engine, small)
    b, cb, eb = check_trees(engine, other)
    first = engine.btc_merkle_root(a, ca, want_mutated=True)
    second = engine.btc_merkle_root(b, cb, want_mutated=True)
    third = engine.btc_merkle_root(a, ca, want_mutated=True)
    assert_roots(engine, first, ea)
    assert_roots(engine, second, eb)
    assert_roots(engine, third, ea)


def test_block_170_and_the_mutated_flag(engine):
    v = KAT["block170"]
    txids = [bytes.fromhex(x)[::-1] for x in v["txids"]]
    a, b, c = (hashlib.sha256(bytes([i])).digest() for i in range(3))
    trees = [txids, [a, b, c], [a, b, c, c], [a, b, a, b], [a, a], [a], [a, b, c, a, b, c]]
    leaves, counts, expected = check_trees(engine, trees)
    roots, mutated = engine.btc_merkle_root(leaves, counts, want_mutated=True)
    got = digests32(engine, roots)
    assert got == [r for r, _ in expected] and got[0][::-1].hex() == v["merkle_root"]
    assert got[1] == got[2]                                                       # CVE-2012-2459: the duplicated last transaction leaves the root as it was ...
    assert flags(mutated) == [0, 0, 1, 1, 1, 0, 0] == [int(m) for _, m in expected]  # ... and only the flag tells; [a, b, a, b]: the equal pair is one level up


def test_no_tree_is_no_work(engine):
    assert engine.btc_merkle_root(engine.empty(0), []).shape[0] == 0


# ---- 3. BIP-341 script paths
TAPLEAF_LENS = [0, 1, 34, 252, 253, 300, 600, 65536]
# around every shape of the tail: prefix + remainder at 55 | 56 (one or two tail blocks) and at 63 | 64 (the 0x80 in the first or the second), for 2, 4 and 6 prefix bytes
TAIL_LENS = [53, 54, 61, 62, 63, 64, 117, 118, 127, 128, 256 + 51, 256 + 52, 256 + 59, 256 + 60, 256 + 63, 320, 65535, 65536 + 49, 65536 + 50, 65536 + 57, 65536 + 58, 65536 + 63,
             65536 + 64]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("lens", [TAPLEAF_LENS, TAIL_LENS], ids=["issue", "tails"])
def test_tapleaf_hashes_equal_the_model(engine, lens, offset):
    rng = random.Random(6 + offset)
    stride = 65536 + 64
    scripts = [rng.randbytes(length) for length in lens]
    versions = [0xc0 + 2 * (i % 7) for i in range(len(lens))]
    view = rows(engine, filled(scripts, stride, 0xA5), stride, offset, len(lens), stride)
    got = engine.tapleaf_hash(view, lens_of(engine, lens), bytes_of(engine, versions))
    assert digests32(engine, got) == [model.tapleaf_hash(s, v) for s, v in zip(scripts, versions)]
    got = engine.tapleaf_hash(view, lens_of(engine, lens), 0xc4)
    assert digests32(engine, got) == [model.tapleaf_hash(s, 0xc4) for s in scripts]


def test_tapleaf_hashes_of_equal_lengths_and_the_bip341_vector(engine):
    v = KAT["bip341_script"]
    script = bytes.fromhex(v["script"])
    others = [random.Random(7).randbytes(len(script)) for _ in range(66)]
    view = rows(engine, b"".join([script] + others), len(script), 0, 67, len(script))
    got = digests32(engine, engine.tapleaf_hash(view, None, v["leaf_version"]))
    assert got[0].hex() == v["leaf_hash"] and got == [model.tapleaf_hash(s) for s in [script] + others]


def control_rows(engine, blocks, width, offset=0):
    return rows(engine, b"".join(b + bytes(width - len(b)) for b in blocks), width, offset, len(blocks), width)


def script_rows(engine, scripts):
    width = max(len(s) for s in scripts)
    return rows(engine, filled(scripts, width, 0), width, 0, len(scripts), width), lens_of(engine, [len(s) for s in scripts])


def test_a_taptree_of_five_leaves_and_its_script_path_spends(engine):
    rng = random.Random(8)
    A, B, C_, D, E = ((rng.randbytes(length), 0xc0) for length in (34, 1, 300, 70, 253))
    root, leaves = model.taptree((A, (B, (C_, (D, E)))))
    assert [len(p) for _, _, p in leaves] == [1, 2, 3, 4, 4]
    px = btc_model.mul_g(0x1234567)[0]
    qx, parity = btc_model.taproot_tweak_pubkey(px, int.from_bytes(root, "big"))
    # every leaf's path reaches the root, and the root gives the output key
    leaf = engine.tapleaf_hash(*script_rows(engine, [s for s, _, _ in leaves]), 0xc0)
    paths = control_rows(engine, [b"".join(p) for _, _, p in leaves], 128)
    roots, ok = engine.taproot_merkle_path(leaf, paths, bytes_of(engine, [len(p) for _, _, p in leaves]))
    assert digests32(engine, roots) == [root] * 5 and flags(ok) == [1] * 5
    q, par, tok = engine.taproot_tweak_pubkey(up(engine, [px] * 5), roots)
    assert arr_to_ints(engine.to_numpy(q)) == [qx] * 5 and flags(par) == [parity] * 5 and flags(tok) == [1] * 5
    # the spends: five good ones, then one bit flipped in a script, a path node, the control byte's parity bit, the output key
    cases = [(qx, model.control_block(px, parity, v, p), s) for s, v, p in leaves]
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]
    cases.append((qx, cases[2][1], flip(cases[2][2], 299)))
    cases.append((qx, flip(cases[3][1], 33 + 32 + 5), cases[3][2]))
    cases.append((qx, bytes([cases[4][1][0] ^ 1]) + cases[4][1][1:], cases[4][2]))
    cases.append((qx ^ (1 << 77), cases[0][1], cases[0][2]))
    expected = [int(model.script_path_ok(q_, cb, s)) for q_, cb, s in cases]
    assert expected == [1] * 5 + [0] * 4
    got = engine.taproot_script_path_ok(up(engine, [q_ for q_, _, _ in cases]), control_rows(engine, [cb for _, cb, _ in cases], 33 + 128),
                                        bytes_of(engine, [(len(cb) - 33) // 32 for _, cb, _ in cases]), *script_rows(engine, [s for _, _, s in cases]))
    assert flags(got) == expected


@pytest.mark.parametrize("offset", [0, 1])
def test_paths_of_every_depth_in_one_wave(engine, offset):
    """Depths 0 ... 128 mixed, so every wave mixes trip counts; depth 129 is refused; one path holds a node equal to the running hash."""
    rng = random.Random(9 + offset)
    depths = [(37 * i) % 129 for i in range(129)] + [129, 2, 255]
    leaves = [rng.randbytes(32) for _ in depths]
    paths = [[rng.randbytes(32) for _ in range(d if d <= 128 else 0)] for d in depths]
    paths[130][1] = model.tapbranch_hash(leaves[130], paths[130][0])                # a = b: the pair is (k, k)
    expected = [model.merkle_path_root(k, p) if d <= 128 else None for k, p, d in zip(leaves, paths, depths)]
    view = control_rows(engine, [b"".join(p) for p in paths], 128 * 32, offset)
    roots, ok = engine.taproot_merkle_path(up32(engine, leaves), view, bytes_of(engine, depths))
    assert flags(ok) == [int(e is not None) for e in expected]
    assert digests32(engine, roots) == [e if e is not None else bytes(32) for e in expected]
    assert expected[130] == model.tagged_hash("TapBranch", paths[130][1] * 2)
    # one depth for every lane
    roots, ok = engine.taproot_merkle_path(up32(engine, leaves[:3]), view[:3, :64], 0)
    assert digests32(engine, roots) == leaves[:3] and flags(ok) == [1] * 3
    roots, ok = engine.taproot_merkle_path(up32(engine, leaves[:3]), view[:3], 129)
    assert digests32(engine, roots) == [bytes(32)] * 3 and flags(ok) == [0] * 3


def test_the_bip341_vector_end_to_end(engine):
    v = KAT["bip341_script"]
    script, px, qx = bytes.fromhex(v["script"]), int(v["internal_key"], 16), int(v["output_key"], 16)
    view, lens = script_rows(engine, [script])
    leaf = engine.tapleaf_hash(view, lens, v["leaf_version"])
    root, ok = engine.taproot_merkle_path(leaf, control_rows(engine, [b""], 32), 0)
    assert digests32(engine, root)[0].hex() == v["leaf_hash"] and flags(ok) == [1]
    q, parity, tok = engine.taproot_tweak_pubkey(up(engine, [px]), root)
    assert arr_to_ints(engine.to_numpy(q)) == [qx] and flags(parity) == [v["parity"]] == [1] and flags(tok) == [1]
    control = model.control_block(px, v["parity"], v["leaf_version"], [])
    assert flags(engine.taproot_script_path_ok(up(engine, [qx]), control_rows(engine, [control], 33), bytes_of(engine, [0]), view, lens)) == [1]
