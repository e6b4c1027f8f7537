"""PBKDF2-HMAC-SHA-512 and the BIP-39 seed, the part that needs no GPU: the two entry points are declared, exported and callable from C99
(tests/c/bip39_caller.c); the host model the GPU tests take their expected values from (tools/pbkdf2_model.py, written from RFC 8018 over hmac) gives every
value of tests/golden/bip39_vectors.json and equals hashlib.pbkdf2_hmac -- an implementation it does not call -- around every boundary of the key block, the
salt's padding and the output blocks; the four kernels exist in the shipped gfx950 listing without scratch memory or spills; the loop's body is the size
profiles/r11/bip39_listing.json says and one of its two compressions is no larger than the compression's committed figure; the kernels keep the passwords, the
salts, the workspace state and the output out of every branch condition, address and lane mask (tools/ct_check.py check_secret_flow) with no declassified bit,
while the analysis refuses a planted branch on one bit of U; and the host layer zeroes the workspace behind the slices whatever the launches said.
The listings are read for kernel names, resource lines, instruction counts and control flow only."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip32_model           # noqa: E402
import capi_secret_shape     # noqa: E402
import ct_check              # noqa: E402
import keccak_listing        # noqa: E402  (the listing reader: any unit's path)
import pbkdf2_model as model  # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "bip39_vectors.json")))
COMMITTED = json.load(open(os.path.join(ROOT, "profiles", "r11", "bip39_listing.json")))
COMPRESSION = json.load(open(os.path.join(ROOT, "profiles", "r10", "bip32_listing.json")))["sha512_compression_valu"]
NEW_SYMBOLS = ("ecsimd_hip_pbkdf2_hmac_sha512", "ecsimd_hip_bip39_seed")
KERNELS = ("k_pbkdf2<1, 1>", "k_pbkdf2<1, 0>", "k_pbkdf2<0, 1>", "k_pbkdf2<0, 0>")
# k_pbkdf2(pw, pw_bytes, pw_stride, pw_lens, salt, salt_bytes, salt_stride, salt_lens, pre, pre_bytes, aligned, block_first, loops, ws, units, out, dk_bytes,
# out_stride, n).  Secret: the passwords, the salts, the workspace, the output.  Public: both lens arrays and every scalar.
SECRET_ARGS = [0, 4, 13, 15]
MANGLED = ("k_pbkdf2ILb1ELb1E", "k_pbkdf2ILb1ELb0E", "k_pbkdf2ILb0ELb1E", "k_pbkdf2ILb0ELb0E")


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def listing(built):
    """({kernel: figures}, text) of the new unit."""
    path = os.path.join(ROOT, "build", "csrc", "k_pbkdf2-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    assert os.path.getmtime(path) >= os.path.getmtime(os.path.join(CSRC, "k_pbkdf2.hip")), path
    return {keccak_listing.short(k): v for k, v in keccak_listing.kernels(path).items()}, open(path).read()


# ---- the C ABI
def test_the_two_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    from ecsimd_amd import Engine
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
        assert callable(getattr(Engine, s[len("ecsimd_hip_"):]))
    assert callable(Engine.bip39_master)
    hdr = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    slice_ = int(re.search(r"enum \{ ECSIMD_HIP_PBKDF2_SLICE = (\d+) \};", hdr).group(1))
    assert 2048 <= slice_ <= 1 << 14                              # BIP-39 is one launch; tests/test_gpu_bip39.py's slice test stays within seconds of hashlib time
    assert "NFKD" in hdr and "word list" in hdr and "checksum" in hdr


def test_the_c99_caller_compiles_and_links(built, tmp_path):
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "bip39_caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "bip39_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in NEW_SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s


@pytest.mark.gpu
def test_the_c99_caller_runs(built, tmp_path):
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "bip39_caller"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "bip39_caller.c"), "-o", str(exe), "-L", libdir, "-lecsimd_hip",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bip39_caller ok" in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]


# ---- the host model
def test_every_fixture_value_equals_the_model_and_hashlib():
    for name in ("trezor", "empty_passphrase", "long_sentence"):
        v = KAT[name]
        m, p = v["mnemonic"].encode(), v["passphrase"].encode()
        assert model.bip39_seed(m, p).hex() == v["seed"] == hashlib.pbkdf2_hmac("sha512", m, b"mnemonic" + p, 2048, 64).hex(), name
    assert len(KAT["long_sentence"]["mnemonic"]) == KAT["long_sentence"]["bytes"] > 128 and len(KAT["long_sentence"]["mnemonic"].split(" ")) == 24
    assert KAT["trezor"]["seed"].startswith("c55257c360c07c72") and KAT["empty_passphrase"]["seed"].startswith("5eb00bbddcf06908")
    k, _ = bip32_model.master(bytes.fromhex(KAT["trezor"]["seed"]))
    assert "%064x" % k == KAT["trezor"]["master_k"] == "cbedc75b0d6412c85c79bc13875112ef912fd1e756631b5a00330866f22ff184"
    v = KAT["pbkdf2_password_salt_1"]
    args = (v["password"].encode(), v["salt"].encode(), v["iterations"], v["dk_bytes"])
    assert model.pbkdf2_hmac_sha512(*args).hex() == v["dk"] == hashlib.pbkdf2_hmac("sha512", *args).hex()


def test_the_model_does_not_call_what_it_is_compared_with():
    src = open(os.path.join(ROOT, "tools", "pbkdf2_model.py")).read()
    code = re.sub(r'""".*?"""', "", src, flags=re.S)
    assert "pbkdf2_hmac(" not in code and "hmac.new(" in code


def test_the_model_equals_hashlib_on_the_sweep():
    for plen in (0, 1, 127, 128, 129, 215):
        pw = bytes((5 * i + plen) & 0xff for i in range(plen))
        for slen in (0, 1, 107, 108, 123, 124, 125, 240):
            salt = bytes((3 * i + slen) & 0xff for i in range(slen))
            for c in (1, 2, 3):
                for dk in (1, 63, 64, 65, 200):
                    assert model.pbkdf2_hmac_sha512(pw, salt, c, dk) == hashlib.pbkdf2_hmac("sha512", pw, salt, c, dk), (plen, slen, c, dk)


# ---- the shipped listing
def test_every_new_kernel_exists_without_scratch_or_spills(listing):
    kernels, asm = listing
    assert sorted(kernels) == sorted(KERNELS), sorted(kernels)
    blocks = re.split(r"\n  - \.agpr_count:", asm[asm.index(".amdgpu_metadata"):])[1:]
    assert len(blocks) == len(kernels)
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", b), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", b), name
        assert re.search(r"\.group_segment_fixed_size:\s+0\b", b), name                    # no LDS
    assert all(k["scratch"] == 0 and k["vgprs"] <= 256 for k in kernels.values())
    assert "k_pbkdf2.hip" in open(os.path.join(CSRC, "Makefile")).read() and COMMITTED["private_segment_fixed_size"] == 0


def test_the_loop_body_is_the_size_the_profile_says(listing):
    """k_pbkdf2<0, 0> is the slice in the middle: loads, THE loop, stores -- one loop, whose body is two compressions and the XOR into T, without a memory access."""
    kernels, _ = listing
    k = kernels["k_pbkdf2<0, 0>"]
    assert k["branches"] == ["exit", "guard", "loop"], k["branches"]
    print("loop body valu", k["loop_valu"], "committed", COMMITTED["loop_valu"], "vgprs", k["vgprs"], "compression", COMPRESSION)
    assert k["loop_vmem"] == 0
    assert abs(k["loop_valu"] - COMMITTED["loop_valu"]) <= 0.05 * COMMITTED["loop_valu"]
    assert k["loop_valu"] / 2 <= 1.05 * COMPRESSION and COMMITTED["loop_valu"] / 2 <= COMPRESSION     # half of every tail block is constants
    assert k["vgprs"] == COMMITTED["loop_kernel_vgprs"] or abs(k["vgprs"] - COMMITTED["loop_kernel_vgprs"]) <= 8


# ---- the secret flow
def test_the_kernels_keep_the_secrets_out_of_control_flow_and_addresses(listing):
    _, asm = listing
    for kernel in MANGLED:
        rep = ct_check.check_secret_flow(asm, kernel, secret_args=SECRET_ARGS)
        assert rep["secret_loads"] >= 16 and not rep["secret_scratch"] and not rep["secret_lds"], kernel
        assert rep["public_branches"] >= 2, kernel                                          # the batch's tail and the loop


def test_the_call_wipes_its_workspace_on_every_path():
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                  # (the one wipe of the workspace is still the shared one)
    body = capi_secret_shape.function(src, "int pbkdf2_derive(")
    assert "hipMemcpy" not in body and "Synchronize" not in body                             # nothing is read back
    # the block is sized and placed by one carve, and only a sliced derivation has one
    assert "ensure_workspace(ctx, pbkdf2_plan(nullptr, chunk * group).bytes)" in body and "L = pbkdf2_plan(ctx->workspace, chunk * group);" in body
    assert "const bool sliced = iterations > slice;" in body
    launches = body[body.index("FOR_CHUNKS(first"):]
    assert launches.count("launch::") == 1 and launches.count("wipe_workspace(") == 1
    # behind the slices of a group of units: the wipe, unconditionally where a workspace was used, fed with whatever the launches said -- and no way out in between
    between = launches[launches.index("launch::pbkdf2_hmac_sha512("):launches.index("wipe_workspace(")]
    assert "return" not in between and "break" not in between and "continue" not in between
    assert "err = sliced ? wipe_workspace(ctx, L.bytes, hipGetLastError()) : hipGetLastError();" in launches
    assert launches.count("return") == 1 and 'fail(ctx, err, "pbkdf2_hmac_sha512 launch")' in launches          # the one way out, behind the loops
    # both entry points are that function and nothing else
    for head in ("int ecsimd_hip_pbkdf2_hmac_sha512(", "int ecsimd_hip_bip39_seed("):
        entry = capi_secret_shape.function(src, head)
        assert entry.count("pbkdf2_derive(") == 1 and "launch::" not in entry and "workspace" not in entry, head
    assert "0x6d6e656d6f6e6963ull" in capi_secret_shape.function(src, "int ecsimd_hip_bip39_seed(") and bytes.fromhex("6d6e656d6f6e6963") == b"mnemonic"


# a planted `return` skips the stores behind it: one bit of U after the loop, in every instance
PLANT_ANCHOR = "  if constexpr (LAST) {\n    const uint32_t take"
PLANT = "  if (S.u.h[3] & 4ull) return;\n"


def test_the_analysis_refuses_a_planted_branch_on_a_secret_bit(tmp_path):
    src = open(os.path.join(CSRC, "k_pbkdf2.hip")).read()
    assert src.count(PLANT_ANCHOR) == 1
    unit, out = tmp_path / "planted.hip", tmp_path / "planted.s"
    unit.write_text(src.replace(PLANT_ANCHOR, PLANT + PLANT_ANCHOR))
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, str(unit), "-o", str(out)], check=True, capture_output=True,
                   timeout=900)
    asm = out.read_text()
    for kernel in MANGLED:
        with pytest.raises(ct_check.Violation) as exc:
            ct_check.check_secret_flow(asm, kernel, secret_args=SECRET_ARGS)
        assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
