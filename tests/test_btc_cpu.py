"""Bitcoin hashes and Taproot key tweaks, the part that needs no GPU: the seven entry points are declared, exported and callable from C99; the host model the
GPU tests take their expected values from (tools/btc_model.py) gives the published known answers of tests/golden/btc_vectors.json; the TapTweak midstate in the
device source is hashlib's; the new kernels exist in the shipped gfx950 listing without scratch memory, the RIPEMD-160 compression is the size
profiles/r09/btc_listing.json says; and the secret-key kernel keeps d, the affine d G and d_out out of every branch condition, address and lane mask
(tools/ct_check.py check_secret_flow) with no declassified bit, while the analysis refuses a planted branch on one bit of d_out or of y's parity."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model        # noqa: E402
import btc_model as model  # noqa: E402
import capi_secret_shape   # noqa: E402
import ct_check            # noqa: E402
import keccak_listing      # noqa: E402  (the listing reader: any unit's path)

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "btc_vectors.json")))
COMMITTED = json.load(open(os.path.join(ROOT, "profiles", "r09", "btc_listing.json")))
NEW_SYMBOLS = ("ecsimd_hip_ripemd160", "ecsimd_hip_hash160", "ecsimd_hip_sha256d", "ecsimd_hip_btc_pubkey_hash", "ecsimd_hip_xonly_tweak_add",
               "ecsimd_hip_taproot_tweak_pubkey", "ecsimd_hip_taproot_tweak_seckey")
HASH_KERNELS = ("k_ripemd160<1>", "k_ripemd160<0>", "k_hash160", "k_sha256d", "k_btc_pubkey_hash<1>", "k_btc_pubkey_hash<0>")
TWEAK_KERNELS = ("k_tweak_front<0>", "k_tweak_front<1>", "k_tweak_front<2>", "k_tweak_add", "k_tweak_accept", "k_taproot_seckey<1>", "k_taproot_seckey<0>")
# k_taproot_seckey(gmod, d, merkle_root, xP, yP, d_out, px, ok, n): the gmod is ONE argument by value.  Secret: d, the affine d G, d_out.
SECKEY = {True: "k_taproot_seckeyILb1E", False: "k_taproot_seckeyILb0E"}
SECKEY_SECRETS = [1, 3, 4, 5]


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
def btc_asm(built):
    return open(listing_path("k_btc")).read()


@pytest.fixture(scope="module")
def kernels(built):
    def named(path):
        out = {}
        for k, v in keccak_listing.kernels(path).items():
            m = re.search(r"\d+(k_[a-z0-9_]+?)(?:IL[bi](\d)E)?E", k)
            out[m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")] = v
        return out
    return named(listing_path("k_btc")), {keccak_listing.short(k): v for k, v in keccak_listing.kernels(listing_path("k_keccak")).items()}


# ---- the C ABI
def test_the_seven_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    from ecsimd_amd import Engine
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
        assert callable(getattr(Engine, s[len("ecsimd_hip_"):]))


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_ripemd160(NULL, b, 33, 36, b, 0);
    rc |= ecsimd_hip_hash160(NULL, b, 33, 36, b, 0);
    rc |= ecsimd_hip_sha256d(NULL, b, 0, 0, w, 0);
    rc |= ecsimd_hip_btc_pubkey_hash(NULL, w, w, b, 0, 1);
    rc |= ecsimd_hip_xonly_tweak_add(NULL, w, w, w, b, b, 0);
    rc |= ecsimd_hip_taproot_tweak_pubkey(NULL, w, NULL, w, b, b, 0);
    rc |= ecsimd_hip_taproot_tweak_seckey(NULL, w, NULL, w, NULL, b, 0);
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
    for v in KAT["ripemd160"]:
        assert model.ripemd160((v["msg"] * v["repeat"]).encode()).hex() == v["digest"], v["msg"][:20]
    assert len(KAT["ripemd160"]) == 9 and KAT["ripemd160"][-1]["repeat"] == 10**6
    for v in KAT["hash160"]:
        assert model.hash160(bytes.fromhex(v["msg_hex"])).hex() == v["digest"]
    assert model.btc_pubkey_hash(model.GX, model.GY, True).hex() == KAT["hash160"][0]["digest"] == "751e76e8199196d454941c45d1b3a323f1433bd6"
    assert model.btc_pubkey_hash(model.GX, model.GY, False).hex() == KAT["hash160"][1]["digest"]
    v = KAT["bip341"]
    px = int(v["internal_key"], 16)
    assert v["merkle_root"] is None and model.tap_tweak(px) == int(v["tweak"], 16)
    assert model.taproot_tweak_pubkey(px) == (int(v["output_key"], 16), v["parity"]) == model.xonly_tweak_add(px, int(v["tweak"], 16))


def test_the_padding_is_right_around_the_block_boundaries():
    """The digest changes with every single-byte change and with the length, at the lengths where the padding changes shape; sha256d is hashlib's twice."""
    for length in (54, 55, 56, 63, 64, 65, 119, 120):
        m = bytes((7 * i + length) & 0xff for i in range(length))
        seen = {model.ripemd160(m)}
        for i in range(length):
            c = bytearray(m); c[i] ^= 0x80
            seen.add(model.ripemd160(bytes(c)))
        seen.add(model.ripemd160(m + b"\x00")); seen.add(model.ripemd160(m[:-1])); seen.add(model.ripemd160(m + b"\x80"))
        assert len(seen) == length + 4, length
        assert model.sha256d(m) == hashlib.sha256(hashlib.sha256(m).digest()).digest()
        assert model.hash160(m) == model.ripemd160(hashlib.sha256(m).digest())


def test_the_tweaked_secret_key_belongs_to_the_tweaked_public_key():
    ds = [d for d in range(3, 40) if model.mul_g(d)[1] % 2 == 0][:2] + [d for d in range(3, 40) if model.mul_g(d)[1] % 2 == 1][:2]
    assert len(ds) == 4
    for d in ds:
        for root in (None, 0x1234567890abcdef << 100):
            d_out, px = model.taproot_tweak_seckey(d, root)
            assert px == model.mul_g(d)[0]
            q = model.mul_g(d_out)
            assert (q[0], q[1] & 1) == model.taproot_tweak_pubkey(px, root)
            msg = b"key path spend %d" % d
            spx, r, s = bip340_model.sign(d_out, msg, 5)
            assert spx == q[0] and bip340_model.verify(q[0], msg, r, s)
    # t = 0 (which no hash gives): Q = P
    assert model.xonly_tweak_add(model.GX, 0) == (model.GX, 0)


def test_the_model_refuses_what_the_device_refuses():
    for bad in (0, model.N, model.N + 1, 2**256 - 1):
        assert model.taproot_tweak_seckey(bad) is None and model.taproot_tweak_seckey(bad, 7) is None
    for bad in (5, model.P, model.P + 1, 2**256 - 1):                           # x = 5: x^3 + 7 is not a square
        assert model.taproot_tweak_pubkey(bad) is None and model.xonly_tweak_add(bad, 1) is None
    assert model.xonly_tweak_add(model.GX, model.N) is None and model.xonly_tweak_add(model.GX, 2**256 - 1) is None
    assert model.xonly_tweak_add(model.GX, model.N - 1) is None                 # G - G
    assert model.xonly_tweak_add(model.GX, 1) == (model.mul_g(2)[0], model.mul_g(2)[1] & 1)      # G + G


def test_the_midstate_in_the_device_source_is_hashlibs():
    src = open(os.path.join(CSRC, "k_btc.hip")).read()
    row = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", re.search(r"TAPTWEAK_MID\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1))]
    assert row == bip340_model.midstate("TapTweak") == [int(x, 16) for x in KAT["taptweak_midstate"]]
    assert re.search(r'tag = "TapTweak"', src) and model.TAG == "TapTweak"
    t = hashlib.sha256(b"TapTweak").digest()
    for data in (bytes(32), bytes(range(64))):
        assert bip340_model.finish_from_midstate(row, data) == hashlib.sha256(t + t + data).digest()


# ---- the shipped listing
def test_every_new_kernel_exists_without_scratch_or_spills(btc_asm, kernels):
    btc, _ = kernels
    assert sorted(btc) == sorted(HASH_KERNELS + TWEAK_KERNELS), sorted(btc)
    meta = btc_asm[btc_asm.index(".amdgpu_metadata"):]
    blocks = re.split(r"\n  - \.agpr_count:", meta)[1:]
    assert len(blocks) == len(btc)
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", b), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", b), name
    assert all(k["scratch"] == 0 for k in btc.values())
    assert "k_btc.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_hash_kernels_touch_no_lds(btc_asm):
    for mangled in ("k_ripemd160ILb1E", "k_ripemd160ILb0E", "9k_hash160", "9k_sha256d", "k_btc_pubkey_hashILb1E", "k_btc_pubkey_hashILb0E"):
        body = "\n".join(i for _, _, insts in ct_check.parse_function(btc_asm, mangled) for i in insts)
        assert body and not re.search(r"^ds_", body, re.M), mangled
        meta = [b for b in re.split(r"\n  - \.agpr_count:", btc_asm[btc_asm.index(".amdgpu_metadata"):])[1:] if mangled in b]
        assert len(meta) == 1 and re.search(r"\.group_segment_fixed_size:\s+0\b", meta[0]), mangled


def test_the_ripemd160_compression_is_the_size_the_profile_says(kernels):
    """The VALU instructions between the labels of k_ripemd160's block loop -- sixteen word loads (or their assembly from bytes) and ONE compression: at most
    160 steps x 9 with word loads, and within 5 % of the committed figure either way."""
    btc, _ = kernels
    got = btc["k_ripemd160<1>"]["loop_valu"]
    print("loop_valu", got, btc["k_ripemd160<0>"]["loop_valu"])
    assert got <= 1440
    assert abs(got - COMMITTED["ripemd160_compression_valu"]) <= 0.05 * COMMITTED["ripemd160_compression_valu"]
    assert abs(btc["k_ripemd160<0>"]["loop_valu"] - COMMITTED["ripemd160_compression_valu_byte_loads"]) <= 0.05 * COMMITTED["ripemd160_compression_valu_byte_loads"]


def test_a_compressed_key_hash_is_fewer_instructions_than_an_ethereum_address(kernels):
    btc, keccak = kernels
    assert btc["k_btc_pubkey_hash<1>"]["valu"] < keccak["k_eth_address<0>"]["valu"]
    assert btc["k_btc_pubkey_hash<1>"]["branches"] == ["exit"] and btc["k_btc_pubkey_hash<0>"]["branches"] == ["exit"]


# ---- the secret flow
def test_the_seckey_kernel_keeps_the_secrets_out_of_control_flow_and_addresses(btc_asm):
    for has_root, kernel in SECKEY.items():
        rep = ct_check.check_secret_flow(btc_asm, kernel, secret_args=SECKEY_SECRETS)
        assert rep["secret_loads"] >= 5 and not rep["secret_scratch"] and not rep["secret_lds"]      # d and x(d G): two 16-byte loads each; y(d G): at least its low half
        assert rep["public_branches"] >= 1                                                             # the batch's tail, px == NULL
        ct_check.check_secret_flow(btc_asm, kernel, secret_args=SECKEY_SECRETS + [2])                 # ... and with the merkle root named secret as well


def test_the_seckey_call_runs_the_constant_time_comb_and_wipes_its_workspace():
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                 # the constant-time comb, the inversion, the unconditional wipe: one copy of each in capi.hip
    # the shared product once per chunk over sign_plan's five arrays (the Jacobian product, x, y), wiped by that total
    body = capi_secret_shape.check_secret_entry(src, "int ecsimd_hip_taproot_tweak_seckey(", products=1)
    assert "sign_plan(ctx->workspace, chunk, true)" in body and "secret_base_product(ctx, curve, d + 4 * first, L.j, L.rx, L.ry, m)" in body
    layout = capi_secret_shape.function(src, "sign_layout sign_plan(")
    assert layout.count("carve_jacobian(c, n)") == 1 and layout.count("carve_limbs(c, n)") == 2 and "L.bytes = c.bytes" in layout     # 5 x 32 B per element, as before
    sign = capi_secret_shape.function(src, "int ecsimd_hip_schnorr_sign(")
    assert "secret_base_product(ctx, curve, d + 4 * first, j, xP, yP, m)" in sign                    # the same product as schnorr_sign's for d G


PLANTS = {
    # one bit of d_out
    "d_out": ("  fe_store(dout, i, sum);\n", "  if (sum.w[3] & 4u) okv[i] = 1;\n"),
    # the parity of y(d G)
    "parity": ("  fe xP = fe_load(xPv, i);\n", "  if ((uint32_t)yPv[4 * i] & 1u) okv[i] = 1;\n"),
}


def test_the_analysis_refuses_a_planted_branch_on_a_secret_bit(tmp_path):
    src = open(os.path.join(CSRC, "k_btc.hip")).read()
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    texts = {"shipped": src}
    for name, (anchor, plant) in PLANTS.items():
        assert src.count(anchor) == 1, name
        texts[name] = src.replace(anchor, plant + anchor)
    for name, text in texts.items():
        unit, out = tmp_path / f"{name}.hip", tmp_path / f"{name}.s"
        unit.write_text(text)
        subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=900)
        asm = out.read_text()
        for kernel in SECKEY.values():
            if name == "shipped":
                ct_check.check_secret_flow(asm, kernel, secret_args=SECKEY_SECRETS)
            else:
                with pytest.raises(ct_check.Violation) as exc:
                    ct_check.check_secret_flow(asm, kernel, secret_args=SECKEY_SECRETS)
                assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
