"""Per-lane lengths, Merkle roots and Taproot script paths, the part that needs no GPU: the seven entry points are declared, exported, callable from C99 and have
their Engine methods; the host model the GPU tests take their expected values from (tools/btc_tree_model.py) gives the published values of
tests/golden/btc_tree_vectors.json; the TapLeaf and TapBranch midstates in the device source are hashlib's; the new kernels exist in the shipped gfx950 listing
without scratch memory, spills or LDS, and the block loops of the per-lane kernels close on the lanes' own mask; bad arguments are refused before any device
is touched."""
import ctypes as C
import hashlib
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model             # noqa: E402
import btc_model                # noqa: E402
import btc_tree_model as model  # noqa: E402
import keccak_listing           # noqa: E402  (the listing reader: any unit's path)

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "btc_tree_vectors.json")))
NEW_SYMBOLS = ("ecsimd_hip_sha256_lens", "ecsimd_hip_sha256d_lens", "ecsimd_hip_hash160_lens", "ecsimd_hip_ripemd160_lens", "ecsimd_hip_btc_merkle_root",
               "ecsimd_hip_tapleaf_hash", "ecsimd_hip_taproot_merkle_path")
LENS_KERNELS = ("k_sha256_lens<1, 0>", "k_sha256_lens<0, 0>", "k_sha256_lens<1, 1>", "k_sha256_lens<0, 1>", "k_sha256_lens<1, 2>", "k_sha256_lens<0, 2>",
                "k_ripemd160_lens<1>", "k_ripemd160_lens<0>")
TREE_KERNELS = ("k_merkle_level", "k_tapleaf_hash<1>", "k_tapleaf_hash<0>", "k_taproot_merkle_path<1>", "k_taproot_merkle_path<0>")
PER_LANE_LOOPS = LENS_KERNELS + TREE_KERNELS[1:]
ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


def listing_path(unit):
    path = os.path.join(ROOT, "build", "csrc", unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    assert os.path.getmtime(path) >= os.path.getmtime(os.path.join(CSRC, unit + ".hip")), path
    return path


def kernel_name(mangled):
    """k_name or k_name<template arguments> of a kernel's symbol; any other symbol as it is"""
    m = re.search(r"\d+(k_[a-z0-9_]+?)(I.*?E)?Ev?P", mangled)
    if not m:
        return mangled
    args = re.findall(r"L[ib](\d+)E", m.group(2) or "")
    return m.group(1) + ("<" + ", ".join(args) + ">" if args else "")


def closing_branches(path):
    """{kernel: [the opcode of every backward conditional branch]}: the branches that close its loops."""
    out, name, at, labels = {}, None, 0, {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, at, labels = kernel_name(m.group(1)), 0, {}
            out[name] = []
            continue
        if name is None:
            continue
        if ".end_amdhsa_kernel" in line:
            name = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            labels[m.group(1)] = at
            continue
        t = line.strip()
        if not t or t.startswith((";", ".")):
            continue
        at += 1
        if t.startswith("s_cbranch") and t.split()[1] in labels:              # a label already seen: the branch goes back
            out[name].append(t.split()[0])
    return out


# ---- the C ABI
def test_the_entry_points_are_declared_exported_and_have_engine_methods(built):
    from ecsimd_amd.engine import declared_symbols
    from ecsimd_amd import Engine
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
    for name in ("sha256", "sha256d", "hash160", "ripemd160"):
        assert inspect.signature(getattr(Engine, name)).parameters["lens"].default is None, name
    for name in ("btc_merkle_root", "tapleaf_hash", "taproot_merkle_path", "taproot_script_path_ok"):
        assert callable(getattr(Engine, name)), name
    assert list(inspect.signature(Engine.taproot_script_path_ok).parameters)[1:] == ["qx", "control_blocks", "depths", "scripts", "lens"]
    assert inspect.signature(Engine.btc_merkle_root).parameters["want_mutated"].default is False
    assert inspect.signature(Engine.tapleaf_hash).parameters["leaf_version"].default == 0xc0


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; uint32_t* l = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_sha256_lens(NULL, b, 0, 200, l, w, 0);
    rc |= ecsimd_hip_sha256d_lens(NULL, b, 0, 200, l, w, 0);
    rc |= ecsimd_hip_hash160_lens(NULL, b, 0, 200, l, b, 0);
    rc |= ecsimd_hip_ripemd160_lens(NULL, b, 33, 36, NULL, b, 0);
    rc |= ecsimd_hip_btc_merkle_root(NULL, w, w, 0, w, NULL);
    rc |= ecsimd_hip_tapleaf_hash(NULL, b, 34, 34, NULL, NULL, 0xc0, w, 0);
    rc |= ecsimd_hip_taproot_merkle_path(NULL, w, b, 4096, b, 0, w, b, 0);
    return rc;
  }
  return 0;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in NEW_SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s


def test_bad_arguments_are_refused_without_a_device(built):
    """The argument checks stand in front of the first HIP call: a zeroed block in place of a context is enough to reach them (its error text is read back), and
    an empty batch returns before a device is looked for."""
    ctx = C.create_string_buffer(1 << 16)
    built.ecsimd_hip_last_error.restype = C.c_char_p
    words = (C.c_uint64 * 64)()
    a = C.cast(words, C.c_void_p)
    a = C.c_void_p((a.value + 15) // 16 * 16)
    size = C.c_size_t
    merkle = built.ecsimd_hip_btc_merkle_root

    def refused(rc, text):
        assert rc == ERR_BAD_ARG and text in built.ecsimd_hip_last_error(ctx).decode(), (rc, built.ecsimd_hip_last_error(ctx))

    refused(merkle(ctx, a, (C.c_uint64 * 3)(0, 2, 2), size(2), a, None), "an empty tree")
    refused(merkle(ctx, a, (C.c_uint64 * 3)(0, 0, 2), size(2), a, None), "an empty tree")
    refused(merkle(ctx, a, (C.c_uint64 * 3)(0, 2, 1), size(2), a, None), "tree_offsets decrease")
    refused(merkle(ctx, a, None, size(2), a, None), "tree_offsets is null")
    refused(merkle(ctx, None, (C.c_uint64 * 2)(0, 2), size(1), a, None), "leaves is null")
    assert merkle(ctx, None, None, size(0), None, None) == 0                                           # m = 0 succeeds
    assert merkle(None, a, (C.c_uint64 * 2)(0, 2), size(1), a, None) == ERR_BAD_ARG
    for name in ("sha256_lens", "sha256d_lens", "hash160_lens", "ripemd160_lens"):
        call = getattr(built, "ecsimd_hip_" + name)
        refused(call(ctx, a, size(0), size(0), a, a, size(2)), "stride_bytes is 0 with lens")
        refused(call(ctx, None, size(0), size(8), a, a, size(2)), "msg is null")
        refused(call(ctx, a, size(0), size(8), C.c_void_p(a.value + 2), a, size(2)), "lens is not 4-byte aligned")
        refused(call(ctx, a, size(0), size(8), a, None, size(2)), "null")
        refused(call(ctx, a, size(16), size(8), None, a, size(2)), "stride_bytes is smaller than msg_bytes")       # lens = NULL: the equal-length call's checks
        assert call(ctx, a, size(0), size(0), a, a, size(0)) == 0                                      # n = 0 succeeds
    leaf = built.ecsimd_hip_tapleaf_hash
    refused(leaf(ctx, a, size(0), size(0), a, None, C.c_uint32(0xc0), a, size(2)), "stride_bytes is 0 with lens")
    refused(leaf(ctx, a, size(8), size(8), None, None, C.c_uint32(0x1c0), a, size(2)), "leaf_version_all is one byte")
    refused(leaf(ctx, a, size(1 << 32), size(1 << 32), None, None, C.c_uint32(0xc0), a, size(2)), "below 2^32")
    assert leaf(ctx, a, size(8), size(8), None, None, C.c_uint32(0xc0), a, size(0)) == 0
    path = built.ecsimd_hip_taproot_merkle_path
    refused(path(ctx, a, None, size(32), None, C.c_uint32(1), C.c_void_p(a.value + 64), a, size(2)), "path is null")
    refused(path(ctx, a, a, size(32), None, C.c_uint32(1), a, a, size(2)), "root must not alias leaf")
    refused(path(ctx, a, a, size(32), None, C.c_uint32(1), C.c_void_p(a.value + 64), None, size(2)), "ok is null")
    assert path(ctx, a, a, size(32), None, C.c_uint32(1), C.c_void_p(a.value + 64), a, size(0)) == 0


# ---- the host model
def test_the_model_gives_every_fixture_value():
    v = KAT["block170"]
    root, mutated = model.merkle_root([bytes.fromhex(x)[::-1] for x in v["txids"]])
    assert root[::-1].hex() == v["merkle_root"] and not mutated
    v = KAT["bip341_script"]
    script, px = bytes.fromhex(v["script"]), int(v["internal_key"], 16)
    leaf = model.tapleaf_hash(script, v["leaf_version"])
    assert leaf.hex() == v["leaf_hash"] and model.merkle_path_root(leaf, []) == leaf and model.taptree((script, v["leaf_version"])) == (leaf, [(script, 0xc0, [])])
    assert btc_model.taproot_tweak_pubkey(px, int.from_bytes(leaf, "big")) == (int(v["output_key"], 16), v["parity"]) and v["parity"] == 1
    control = model.control_block(px, v["parity"], v["leaf_version"], [])
    assert model.script_path_ok(int(v["output_key"], 16), control, script)
    assert not model.script_path_ok(int(v["output_key"], 16), bytes([control[0] ^ 1]) + control[1:], script)
    assert KAT["tapleaf_midstate"] == ["%08x" % x for x in bip340_model.midstate("TapLeaf")]
    assert KAT["tapbranch_midstate"] == ["%08x" % x for x in bip340_model.midstate("TapBranch")]


def test_the_compact_size_changes_shape_where_bitcoins_does():
    assert model.compact_size(0) == b"\x00" and model.compact_size(252) == b"\xfc"
    assert model.compact_size(253) == b"\xfd\xfd\x00" and model.compact_size(65535) == b"\xfd\xff\xff"
    assert model.compact_size(65536) == b"\xfe\x00\x00\x01\x00" and model.compact_size(2**32 - 1) == b"\xfe\xff\xff\xff\xff"
    for n in (252, 253, 65535, 65536):
        s = bytes(n)
        t = hashlib.sha256(b"TapLeaf").digest()
        assert model.tapleaf_hash(s, 0xc2) == hashlib.sha256(t + t + b"\xc2" + model.compact_size(n) + s).digest()


def test_a_duplicated_last_leaf_keeps_the_root_and_sets_the_flag():
    a, b, c, d = (hashlib.sha256(bytes([i])).digest() for i in range(4))
    dd = lambda x, y: hashlib.sha256(hashlib.sha256(x + y).digest()).digest()
    assert model.merkle_root([a]) == (a, False)
    assert model.merkle_root([a, b, c]) == (dd(dd(a, b), dd(c, c)), False)
    assert model.merkle_root([a, b, c, c]) == (dd(dd(a, b), dd(c, c)), True)
    assert model.merkle_root([a, b, a, b]) == (dd(dd(a, b), dd(a, b)), True)                            # the equal pair is one level up
    assert model.merkle_root([a, b, c, d, a])[1] is False                                             # the odd node is paired with itself: not a real pair


def test_the_taptree_builder_gives_every_leaf_a_path_to_the_root():
    leaves = [(bytes([i]) * (i + 1), 0xc0) for i in range(5)]
    root, out = model.taptree((leaves[0], (leaves[1], (leaves[2], (leaves[3], leaves[4])))))
    assert [len(p) for _, _, p in out] == [1, 2, 3, 4, 4] and [(s, v) for s, v, _ in out] == leaves
    assert all(model.merkle_path_root(model.tapleaf_hash(s, v), p) == root for s, v, p in out)
    assert model.merkle_path_root(root, [root] * 129) is None and model.merkle_path_root(root, [root] * 128) is not None
    assert model.tapbranch_hash(root, out[0][2][0]) == model.tapbranch_hash(out[0][2][0], root)


def test_the_midstates_in_the_device_source_are_hashlibs():
    src = open(os.path.join(CSRC, "k_btc_tree.hip")).read()
    for tag, name, key in (("TapLeaf", "TAPLEAF_MID", "tapleaf_midstate"), ("TapBranch", "TAPBRANCH_MID", "tapbranch_midstate")):
        row = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", re.search(name + r"\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1))]
        assert row == bip340_model.midstate(tag) == [int(x, 16) for x in KAT[key]], tag
        assert 'tag = "%s"' % tag in src
        t = hashlib.sha256(tag.encode()).digest()
        for data in (bytes(32), bytes(range(64)), bytes(range(70))):
            assert bip340_model.finish_from_midstate(row, data) == hashlib.sha256(t + t + data).digest()


# ---- the shipped listing
def test_every_new_kernel_exists_without_scratch_spills_or_lds(built):
    path = listing_path("k_btc_tree")
    asm = open(path).read()
    found = {kernel_name(k): v for k, v in keccak_listing.kernels(path).items()}
    assert sorted(found) == sorted(LENS_KERNELS + TREE_KERNELS), sorted(found)
    blocks = re.split(r"\n  - \.agpr_count:", asm[asm.index(".amdgpu_metadata"):])[1:]
    assert len(blocks) == len(found)
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", b), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", b) and re.search(r"\.sgpr_spill_count:\s+0\b", b), name
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", b), name
    assert all(k["scratch"] == 0 for k in found.values())
    assert not re.search(r"^\s+(ds_|scratch_)", asm, re.M)
    assert "k_btc_tree.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_block_loops_of_the_per_lane_kernels_close_on_the_lanes_own_mask(built):
    """A loop whose trip count is a kernel argument closes on a condition code of a uniform compare (s_cbranch_scc* / s_cbranch_vcc*) and leaves the lane mask
    alone: k_sha256's and k_sha256d's block loops do.  A loop whose trip count is the lane's own takes the finished lanes out of the mask and runs until the
    wave's last lane is done: its closing branch is s_cbranch_execnz.  A structural check, no instruction count."""
    loops = closing_branches(listing_path("k_btc_tree"))
    for k in PER_LANE_LOOPS:
        assert "s_cbranch_execnz" in loops[k], (k, loops[k])
    for unit, kernel in (("k_sha256", "k_sha256"), ("k_btc", "k_sha256d")):
        uniform = closing_branches(listing_path(unit))[kernel]
        assert uniform and all(op.startswith(("s_cbranch_scc", "s_cbranch_vcc")) for op in uniform), (kernel, uniform)
