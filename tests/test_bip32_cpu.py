"""SHA-512, HMAC-SHA-512 and BIP-32 key derivation, the part that needs no GPU: the five entry points are declared, exported and callable from C99; the host
model the GPU tests take their expected values from (tools/bip32_model.py) gives the published BIP-32 vectors of tests/golden/bip32_vectors.json and equals
hashlib / hmac around the padding boundaries; the "Bitcoin seed" midstates in the device source are the model's; the new kernels exist in the shipped gfx950
listing without scratch memory, the SHA-512 compression is the size profiles/r10/bip32_listing.json says and no larger than its plain-uint64_t form; and the
three secret kernels keep the seed, the keys, the chain codes and the affine k_par G out of every branch condition, address and lane mask
(tools/ct_check.py check_secret_flow) with no declassified bit, while the analysis refuses a planted branch on one bit of k_child or of y's parity.
The listings are read for kernel names, resource lines, instruction counts and control flow only."""
import hashlib
import hmac
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip32_model as model  # noqa: E402
import capi_secret_shape     # noqa: E402
import ct_check              # noqa: E402
import keccak_listing        # noqa: E402  (the listing reader: any unit's path)

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "bip32_vectors.json")))
COMMITTED = json.load(open(os.path.join(ROOT, "profiles", "r10", "bip32_listing.json")))
NEW_SYMBOLS = ("ecsimd_hip_sha512", "ecsimd_hip_hmac_sha512", "ecsimd_hip_bip32_master", "ecsimd_hip_bip32_ckd_priv", "ecsimd_hip_bip32_ckd_pub")
SHA512_KERNELS = ("k_sha512<1>", "k_sha512<0>", "k_hmac_sha512<1, 1>", "k_hmac_sha512<1, 0>", "k_hmac_sha512<0, 1>", "k_hmac_sha512<0, 0>")
BIP32_KERNELS = ("k_bip32_master", "k_bip32_ckd_priv<1>", "k_bip32_ckd_priv<0>", "k_bip32_ckd_pub_front", "k_bip32_ckd_pub_accept")
LENGTHS = (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256)
# k_bip32_master(words8, seed, seed_bytes, stride, k, c, ok, n): the words8 is ONE argument by value.  Secret: the seed, k, c.
# k_bip32_ckd_priv(gmod, k_par, c_par, index, index_all, xP, yP, k_child, c_child, ok, n).  Secret: k_par, c_par, the affine k_par G, k_child, c_child.
SECRET = {"k_bip32_masterE": [1, 4, 5], "k_bip32_ckd_privILb1E": [1, 2, 5, 6, 7, 8], "k_bip32_ckd_privILb0E": [1, 2, 5, 6, 7, 8]}


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


@pytest.fixture(scope="module")
def listings(built):
    """({kernel: figures}, text) per new unit."""
    def named(path):
        out = {}
        for k, v in keccak_listing.kernels(path).items():
            m = re.search(r"\d+(k_[a-z0-9_]+?)(?:I((?:L[bi]\d+E)+)E)?E", k)
            out[m.group(1) + ("<%s>" % ", ".join(re.findall(r"L[bi](\d+)E", m.group(2))) if m.group(2) else "")] = v
        return out
    return {unit: (named(listing_path(unit)), open(listing_path(unit)).read()) for unit in ("k_sha512", "k_bip32")}


# ---- the C ABI
def test_the_five_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    from ecsimd_amd import Engine
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
        assert callable(getattr(Engine, s[len("ecsimd_hip_"):]))
    assert callable(Engine.bip32_derive_priv)
    from ecsimd_amd import flags
    hdr = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    assert int(re.search(r"ECSIMD_HIP_BIP32_ALL_HARDENED\s*=\s*(\d+)", hdr).group(1)) == flags.BIP32_ALL_HARDENED


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; uint32_t* i = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_sha512(NULL, b, 33, 36, b, 0);
    rc |= ecsimd_hip_hmac_sha512(NULL, b, 12, 0, b, 33, 36, b, 0);
    rc |= ecsimd_hip_bip32_master(NULL, b, 16, 16, w, w, b, 0);
    rc |= ecsimd_hip_bip32_ckd_priv(NULL, w, w, i, 0, w, w, b, 0, ECSIMD_HIP_BIP32_ALL_HARDENED);
    rc |= ecsimd_hip_bip32_ckd_pub(NULL, w, w, w, NULL, 7u, w, w, w, b, 0);
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


# ---- the host model
def test_the_model_gives_every_fixture_value():
    assert model.sha512(b"abc").hex() == KAT["sha512_abc"]
    nodes = 0
    for name in ("vector1", "vector2", "vector3"):
        v = KAT[name]
        k, c = model.master(bytes.fromhex(v["seed"]))
        assert (k, c) == (int(v["master"]["k"], 16), int(v["master"]["c"], 16)), name
        path = []
        for lv in v.get("chain", []):
            path.append(int(lv["index"], 16))
            assert (path[-1] >= model.HARDENED) == lv["path"].endswith("'")
            k, c = model.ckd_priv(k, c, path[-1])
            assert (k, c) == (int(lv["k"], 16), int(lv["c"], 16)), lv["path"]
            assert model.derive(int(v["master"]["k"], 16), int(v["master"]["c"], 16), path) == (k, c)
            nodes += 1
    assert nodes == 6 and len(bytes.fromhex(KAT["vector2"]["seed"])) == 64
    m = int(KAT["vector1"]["master"]["k"], 16)
    assert model.ser_p(model.mul_g(m)).hex() == KAT["vector1"]["master_pubkey"] and model.fingerprint(m).hex() == KAT["vector1"]["master_fingerprint"] == "3442193e"


def test_the_model_equals_hashlib_around_the_padding_boundaries():
    assert model.IV[0] == 0x6a09e667f3bcc908 and model.K[0] == 0x428a2f98d728ae22 and model.K[79] == 0x6c44198c4a475817      # FIPS 180-4, 4.2.3 and 5.3.5
    for length in LENGTHS:
        m = bytes((7 * i + length) & 0xff for i in range(length))
        assert model.sha512(m) == hashlib.sha512(m).digest(), length
        for klen in (0, 1, 32, 127, 128, 129, 200):
            key = bytes((11 * i + klen) & 0xff for i in range(klen))
            assert model.hmac_sha512(key, m) == hmac.new(key, m, hashlib.sha512).digest(), (klen, length)


def test_ckd_pub_of_the_public_key_is_the_public_key_of_ckd_priv():
    k, c = model.master(bytes.fromhex(KAT["vector1"]["seed"]))
    for index in (0, 1, model.HARDENED - 1):
        child = model.ckd_priv(k, c, index)
        assert model.ckd_pub(model.mul_g(k), c, index) == (model.mul_g(child[0]), child[1])
    assert model.ckd_pub(model.mul_g(k), c, model.HARDENED) is None and model.ckd_pub((0, 0), c, 0) is None
    for bad in (0, model.N, model.N + 1, 2**256 - 1):
        assert model.ckd_priv(bad, c, 0) is None and model.ckd_priv(bad, c, model.HARDENED) is None
    assert model.ckd_priv(1, c, 3) is not None and model.ckd_priv(model.N - 1, c, model.HARDENED + 3) is not None
    assert model.master(bytes(16)) is not None


def test_the_midstates_in_the_device_source_are_the_models():
    src = open(os.path.join(CSRC, "k_bip32.hip")).read()
    inner, outer = model.hmac_midstates(b"Bitcoin seed")
    for name, want in (("SEED_INNER", inner), ("SEED_OUTER", outer)):
        row = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ull", re.search(name + r"\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1))]
        assert row == want, name
    assert model.SEED_KEY == b"Bitcoin seed" and '"Bitcoin seed"' in src
    for seed in (bytes(16), bytes(range(64))):
        assert model.finish(outer, model.finish(inner, seed, 128), 128) == hmac.new(b"Bitcoin seed", seed, hashlib.sha512).digest()
    # ... and the round constants and the initial state of sha512.cuh are FIPS 180-4's, which the model computes from the primes
    hdr = open(os.path.join(CSRC, "sha512.cuh")).read()
    for name, want in (("K[80]", model.K), ("IV[8]", model.IV)):
        body = re.search(re.escape(name) + r"\s*=\s*\{(.*?)\};", hdr, re.S).group(1)
        assert [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ull", body)] == want, name


# ---- the shipped listing
def test_every_new_kernel_exists_without_scratch_or_spills(listings):
    for unit, want in (("k_sha512", SHA512_KERNELS), ("k_bip32", BIP32_KERNELS)):
        kernels, asm = listings[unit]
        assert sorted(kernels) == sorted(want), sorted(kernels)
        blocks = re.split(r"\n  - \.agpr_count:", asm[asm.index(".amdgpu_metadata"):])[1:]
        assert len(blocks) == len(kernels)
        for b in blocks:
            name = re.search(r"\.name:\s+(\S+)", b).group(1)
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", b), name
            assert re.search(r"\.vgpr_spill_count:\s+0\b", b), name
        assert all(k["scratch"] == 0 for k in kernels.values())
        assert unit + ".hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert "sha512.cuh" in open(os.path.join(CSRC, "Makefile")).read() and COMMITTED["private_segment_fixed_size"] == 0


def test_the_sha512_compression_is_the_size_the_profile_says_and_no_larger_than_its_plain_form(listings):
    """One compression = a quarter of k_bip32_ckd_priv<0>, straight-line code of exactly four compressions (profiles/r10/bip32_listing.json says what else that
    charges to the compression): within 5 % of the committed figure, and at most the figure recorded there for the same kernel on plain uint64_t rotations."""
    bip32, _ = listings["k_bip32"]
    k = bip32["k_bip32_ckd_priv<0>"]
    assert k["branches"] == ["exit", "other"] or k["branches"] == ["exit"], k["branches"]            # the batch's tail, index == NULL: no loop left standing
    got = k["valu"] / 4
    print("sha512 compression valu", got, "committed", COMMITTED["sha512_compression_valu"], "naive", COMMITTED["sha512_compression_valu_naive"], "vgprs", k["vgprs"])
    assert abs(got - COMMITTED["sha512_compression_valu"]) <= 0.05 * COMMITTED["sha512_compression_valu"]
    assert got <= COMMITTED["sha512_compression_valu_naive"]
    assert COMMITTED["sha512_compression_valu"] <= COMMITTED["sha512_compression_valu_naive"]
    # the other kernels are whole numbers of compressions: master two, the public front four
    assert bip32["k_bip32_master"]["valu"] < 0.55 * k["valu"] and bip32["k_bip32_ckd_priv<1>"]["valu"] < 1.01 * k["valu"]
    assert "loop" not in bip32["k_bip32_master"]["branches"] and "loop" not in bip32["k_bip32_ckd_priv<1>"]["branches"]


# ---- the secret flow
def test_the_secret_kernels_keep_the_secrets_out_of_control_flow_and_addresses(listings):
    _, asm = listings["k_bip32"]
    for kernel, secrets in SECRET.items():
        rep = ct_check.check_secret_flow(asm, kernel, secret_args=secrets)
        assert rep["secret_loads"] >= 4 and not rep["secret_scratch"] and not rep["secret_lds"], kernel
        assert rep["public_branches"] >= 1, kernel                                                     # the batch's tail


def test_the_priv_call_runs_the_constant_time_comb_and_wipes_its_workspace():
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                 # the constant-time comb, the inversion, the unconditional wipe: one copy of each in capi.hip
    head = "int ecsimd_hip_bip32_ckd_priv("
    # the route with a point multiplication: the shared product once per chunk over sign_plan's five arrays (the Jacobian product, x, y), wiped by that total
    route = capi_secret_shape.check_secret_entry(src, head, products=1, route="ENTER_ANY_SIZE();")
    assert "sign_plan(ctx->workspace, chunk, true)" in route and "secret_base_product(ctx, curve, k_par + 4 * first, L.j, L.rx, L.ry, m)" in route
    layout = capi_secret_shape.function(src, "sign_layout sign_plan(")
    assert layout.count("carve_jacobian(c, n)") == 1 and layout.count("carve_limbs(c, n)") == 2 and "L.bytes = c.bytes" in layout     # 5 x 32 B per element, as before
    # the hardened-only route: decided from the flags and the indices' pointer, one launch, no workspace
    body = capi_secret_shape.function(src, head)
    hardened = body[body.index("if ((flags & ECSIMD_HIP_BIP32_ALL_HARDENED) != 0"):body.index("ENTER_ANY_SIZE();")]
    assert hardened.count("launch::") == 1 and "launch::bip32_ckd_priv(ctx->stream, O.N, k_par, c_par, index, index_all, nullptr, nullptr," in hardened and "return" in hardened
    assert "workspace" not in hardened and "_plan(" not in hardened and "secret_base_product" not in hardened
    assert "hipMemcpy" not in body and "Synchronize" not in body                                        # nothing is read back to choose the route


# a planted `return` skips the stores behind it: a store planted in front of the kernel's own store to the same place would be removed as dead
PLANTS = {
    # one bit of k_child: both instantiations
    "k_child": ("  fe_store(kout, i, sum); fe_store(cout, i, c);\n", "  if (sum.w[3] & 4u) return;\n", ("k_bip32_ckd_privILb1E", "k_bip32_ckd_privILb0E")),
    # the parity of y(k_par G): the instantiation that reads the point
    "parity": ("    x = fe_select(hardened, k, fe_load(xPv, i));\n", "    if ((uint32_t)yPv[4 * i] & 1u) return;\n", ("k_bip32_ckd_privILb1E",)),
}


def test_the_analysis_refuses_a_planted_branch_on_a_secret_bit(tmp_path):
    src = open(os.path.join(CSRC, "k_bip32.hip")).read()
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    texts = {"shipped": src}
    for name, (anchor, plant, _) in PLANTS.items():
        assert src.count(anchor) == 1, name
        texts[name] = src.replace(anchor, plant + anchor)
    for name, text in texts.items():
        unit, out = tmp_path / f"{name}.hip", tmp_path / f"{name}.s"
        unit.write_text(text)
        subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=900)
        asm = out.read_text()
        for kernel, secrets in SECRET.items():
            if name == "shipped" or kernel not in PLANTS[name][2]:
                ct_check.check_secret_flow(asm, kernel, secret_args=secrets)
            else:
                with pytest.raises(ct_check.Violation) as exc:
                    ct_check.check_secret_flow(asm, kernel, secret_args=secrets)
                assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
