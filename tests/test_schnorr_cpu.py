"""BIP-340 Schnorr signatures, the part that needs no GPU: the two entry points are declared, exported and callable from C99; the host model the GPU
tests take their expected values from (tools/bip340_model.py) gives BIP-340's test vectors 0 and 1 and rejects every one-field change of them; the three
tag midstates in the device source are hashlib's; the new kernels exist in the shipped gfx950 listing without scratch memory; the two signing kernels and
the comb and inversion between them keep d, aux, the nonce and both products out of every branch condition, address and lane mask
(tools/ct_check.py check_secret_flow) with no declassified bit, and the analysis refuses a planted branch on one bit of the nonce or of a y's parity."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model as model   # noqa: E402
import capi_secret_shape       # noqa: E402
import ct_check                # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
NEW_SYMBOLS = ("ecsimd_hip_schnorr_verify", "ecsimd_hip_schnorr_sign")
NEW_KERNELS = ("22k_schnorr_verify_front", "16k_schnorr_accept", "15k_schnorr_nonce", "16k_schnorr_finish")
# scalar memory writes and what goes with them are off limits on the machines this runs on, in any letter case, comments and strings included -- which is
# why the words are put together here instead of being written out
FORBIDDEN = re.compile("|".join("s_" + w for w in ("store_" + "dword", "buffer_" + "store", "scratch_" + "store", "atomic_", "buffer_" + "atomic", "dcache_" + "wb", "dcache_" + "discard")), re.I)
# k_schnorr_nonce(order, d, aux, xP, yP, msg, msg_bytes, stride, aligned, k0, n): order is 32 bytes BY VALUE, one argument.
# Secret: d, aux, the affine d G (public once returned, secret until then), the nonce buffer.
NONCE, NONCE_SECRETS = "k_schnorr_nonce", [1, 2, 3, 4, 9]
# k_schnorr_finish(gmod, d, k0, xP, yP, xR, yR, msg, msg_bytes, stride, aligned, px, r, s, ok, n): d, the nonce, both affine products
FINISH, FINISH_SECRETS = "k_schnorr_finish", [1, 2, 3, 4, 5, 6]


def vectors():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.json")))
    out = []
    for c in kat["cases"]:
        sig = bytes.fromhex(c["signature"])
        out.append(dict(d=int(c["secret_key"], 16), px=int(c["public_key"], 16), aux=int(c["aux_rand"], 16), msg=bytes.fromhex(c["message"]),
                        r=int.from_bytes(sig[:32], "big"), s=int.from_bytes(sig[32:], "big")))
    assert len(out) == 2
    return out


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


def listing_of(unit):
    listing = os.path.join(ROOT, "build", "csrc", unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, unit + ".hip")), listing
    return open(listing).read()


@pytest.fixture(scope="module")
def schnorr_asm(built):
    return listing_of("k_schnorr")


# ---- the C ABI
def test_both_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
    from ecsimd_amd import Engine
    for m in ("schnorr_verify", "schnorr_sign"):
        assert callable(getattr(Engine, m))


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_schnorr_verify(NULL, w, b, 32, 32, w, w, b, 0);
    rc |= ecsimd_hip_schnorr_sign(NULL, w, b, 32, 40, NULL, NULL, w, w, b, 0);
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
def test_known_answers_through_the_model():
    """BIP-340 test vectors 0 and 1: the public key and the signature bit for bit, and the signature verifies."""
    for v in vectors():
        assert model.pubkey(v["d"]) == v["px"]
        assert model.sign(v["d"], v["msg"], v["aux"]) == (v["px"], v["r"], v["s"])
        assert model.verify(v["px"], v["msg"], v["r"], v["s"])
    assert model.sign(3, bytes(32)) == model.sign(3, bytes(32), 0)                      # no aux = 32 zero bytes


def test_the_model_rejects_every_one_field_change():
    for v in vectors():
        px, msg, r, s = v["px"], v["msg"], v["r"], v["s"]
        for bit in (0, 1, 77, 255):
            flip = 1 << bit
            assert not model.verify(px ^ flip, msg, r, s)
            assert not model.verify(px, msg, r ^ flip, s)
            assert not model.verify(px, msg, r, s ^ flip)
        for byte in (0, 13, 31):
            m2 = bytearray(msg); m2[byte] ^= 0x10
            assert not model.verify(px, bytes(m2), r, s)
        assert not model.verify(px, msg + b"\x00", r, s) and not model.verify(px, msg[:-1], r, s)
        assert not model.verify(px, msg, r, model.N - s)
        assert not model.verify(px, msg, model.P, s) and not model.verify(px, msg, r, model.N) and not model.verify(model.P, msg, r, s)
    # an odd-R signature (the nonce left as drawn) satisfies the group equation and is still refused
    d, msg = 0xB7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFEF, b"odd R"
    aux = next(a for a in range(64) if model.nonce_point_is_odd(d, msg, a))
    px, r, s = model.sign(d, msg, aux, negate_nonce=False)
    assert not model.verify(px, msg, r, s) and model.verify(px, msg, *model.sign(d, msg, aux)[1:])
    # keys out of range are refused; messages of any length sign and verify
    for bad in (0, model.N, model.N + 1, 2**256 - 1):
        assert model.sign(bad, b"x") is None and model.pubkey(bad) is None
    for length in (0, 1, 33, 55, 64, 100):
        px, r, s = model.sign(5, bytes(range(length)), 9)
        assert model.verify(px, bytes(range(length)), r, s)
    assert model.lift_x(model.P) is None and model.lift_x(5) is None and model.lift_x(model.GX) == (model.GX, model.GY)   # x = 5: x^3 + 7 is not a square


def test_the_midstates_in_the_device_source_are_hashlibs():
    """The literals of k_schnorr.hip = the state after the tag block, and a hash continued from them by the plain compression function = hashlib's."""
    src = open(os.path.join(CSRC, "k_schnorr.hip")).read()
    table = re.search(r"BIP340_MID\[3\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [[int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", row)] for row in re.findall(r"\{([^{}]*)\}", table)]
    assert len(rows) == 3 and all(len(r) == 8 for r in rows)
    order = re.search(r'tag = "BIP0340/(\w+)", "BIP0340/(\w+)", "BIP0340/(\w+)"', src).groups()
    assert tuple("BIP0340/" + t for t in order) == model.TAGS
    for tag, row in zip(model.TAGS, rows):
        assert row == model.midstate(tag), tag
        for length in (0, 1, 32, 55, 56, 64, 96, 119, 120, 200):
            data = hashlib.sha256(b"%d" % length).digest() * 7
            t = hashlib.sha256(tag.encode()).digest()
            assert model.finish_from_midstate(row, data[:length]) == hashlib.sha256(t + t + data[:length]).digest() == model.tagged_hash(tag, data[:length])


# ---- the shipped ISA
def test_new_kernels_exist_and_use_no_scratch(schnorr_asm):
    meta = schnorr_asm[schnorr_asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    assert len(blocks) == len(NEW_KERNELS), sorted(blocks)
    for k in NEW_KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", hit[0]), k
    assert "scratch_" not in schnorr_asm
    assert "k_schnorr.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_hashes_are_the_compressions_the_design_counts(schnorr_asm):
    """~1 500 VALU instructions per compression: the front end and the finishing kernel hold two in their text (the prefix block, the block loop's body), the
    nonce kernel three (the aux hash on top)."""
    for kernel, compressions in (("k_schnorr_verify_front", 2), (NONCE, 3), (FINISH, 2)):
        body = "\n".join(i for _, _, insts in ct_check.parse_function(schnorr_asm, kernel) for i in insts)
        assert len(re.findall(r"^v_alignbit_b32", body, re.M)) >= compressions * 64 * 6, kernel
        assert len(re.findall(r"^v_alignbit_b32", body, re.M)) < (compressions + 1) * 64 * 6 + 200, kernel
        assert not re.search(r"^(ds_|buffer_|flat_)", body, re.M), kernel


def test_no_off_limits_instruction_word_anywhere(schnorr_asm):
    assert not FORBIDDEN.search(schnorr_asm)
    for f in ("k_schnorr.hip", "lift.cuh", "sha256.cuh", "k_sha256.hip", "k_recover.hip", "capi.hip", "kernels.h"):
        assert not FORBIDDEN.search(open(os.path.join(CSRC, f)).read()), f
    for f in ("tools/bip340_model.py", "tests/test_gpu_schnorr.py", "tests/cpp/schnorr_tests.cpp", "include/ecsimd_hip.h", "include/ecsimd/curve_group.h"):
        assert not FORBIDDEN.search(open(os.path.join(ROOT, f)).read()), f


def test_signing_kernels_keep_the_secrets_out_of_control_flow_and_addresses(schnorr_asm):
    rep = ct_check.check_secret_flow(schnorr_asm, NONCE, secret_args=NONCE_SECRETS)
    assert rep["secret_loads"] >= 7 and not rep["secret_scratch"] and not rep["secret_lds"]     # d, aux, x(d G): two 16-byte loads each; y(d G): at least its low half
    assert rep["public_branches"] >= 2                                                           # the batch's tail, aux == NULL, the block loop: public values all
    rep = ct_check.check_secret_flow(schnorr_asm, FINISH, secret_args=FINISH_SECRETS)
    assert rep["secret_loads"] >= 9 and not rep["secret_scratch"] and not rep["secret_lds"]     # d, k0, x(d G), x(k0 G) in full, the two y at least in part
    assert rep["public_branches"] >= 2
    # with the MESSAGE named secret as well nothing changes: its bytes reach no branch and no address (the length and the stride are the call's)
    ct_check.check_secret_flow(schnorr_asm, NONCE, secret_args=NONCE_SECRETS + [5])
    ct_check.check_secret_flow(schnorr_asm, FINISH, secret_args=FINISH_SECRETS + [7])


def test_the_comb_and_the_inversion_between_them_with_d_as_the_scalar(built):
    """What schnorr_sign runs for d G and k0 G on secp256k1: the constant-time 5-bit comb (argument 0 = the scalar: d, then k0; 2-4 = the Jacobian product)
    and the simultaneous inversion that keeps y (every array secret)."""
    asm = listing_of("k_affine_secp256k1")
    rep = ct_check.check_secret_flow(asm, "k_base_windowed_sILi5ELb1ELi256E", secret_args=[0, 2, 3, 4])
    assert rep["secret_loads"] == 2 and not rep["secret_lds"]
    rep = ct_check.check_secret_flow(asm, "k_to_affine_batchedILb1E", secret_args=[0, 1, 2, 3, 4])
    assert rep["secret_loads"] >= 6
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                 # the constant-time comb, the inversion, the unconditional wipe: one copy of each in capi.hip
    # schnorr_sign: the shared product twice (d G, then k0 G over the same Jacobian arrays) inside ONE wiped scope of eight arrays per element
    body = capi_secret_shape.check_secret_entry(src, "int ecsimd_hip_schnorr_sign(", products=2)
    assert "secret_base_product(ctx, curve, d + 4 * first, j, xP, yP, m)" in body and "secret_base_product(ctx, curve, k0, j, xR, yR, m)" in body
    place = body[body.index("auto place = "):body.index("return c;")]
    assert place.count("carve_jacobian(c, chunk)") == 1 and place.count("carve_limbs(c, chunk)") == 5                       # 8 x 32 B per element, as before
    # ECDSA: both entry points go through the one signer per curve kind, and the built-in one through the shared product once: x only (4 arrays) for
    # ecdsa_sign, with y (5 arrays) for ecdsa_sign_recoverable
    for head in ("int ecsimd_hip_ecdsa_sign(", "int ecsimd_hip_ecdsa_sign_recoverable("):
        entry = capi_secret_shape.function(src, head)
        assert len(re.findall(r"\becdsa_sign_builtin\(", entry)) == 1 and len(re.findall(r"\becdsa_sign_registered\(", entry)) == 1, head
        assert "launch::" not in entry and "workspace" not in entry and "hipMemcpy" not in entry and "Synchronize" not in entry, head
    signer = capi_secret_shape.check_secret_entry(src, "int ecdsa_sign_builtin(", products=1)
    assert "sign_plan(ctx->workspace, n, v != nullptr)" in signer and "secret_base_product(ctx, curve, k, L.j, L.rx, L.ry, n)" in signer
    assert "L.ry = keep_y ? carve_limbs(c, n) : nullptr" in capi_secret_shape.function(src, "sign_layout sign_plan(")
    registered = capi_secret_shape.function(src, "int ecdsa_sign_registered(")
    assert "rc = ensure_workspace(ctx, L.bytes);" in registered and "L = gc_plan(ctx->workspace, n);" in registered
    assert re.search(r"^\s*const hipError_t err = wipe_workspace\(ctx, L\.bytes, hipGetLastError\(\)\);", registered, re.M)   # the same unconditional wipe, over gc_plan's total
    assert "hipMemcpy" not in registered and "Synchronize" not in registered


PLANTS = {
    # one bit of the nonce, in the kernel that makes it
    "k0": (NONCE, NONCE_SECRETS, "  fe_store(k0v, i, k0);\n", "  if (k0.w[3] & 4u) k0.w[0] ^= (uint32_t)msg[i * stride];\n"),
    # the parity of y(k0 G), in the kernel that negates the nonce by it
    "parity": (FINISH, FINISH_SECRETS, "  const fe ed = g_mul(g_mul(e, dd, M), g_words(M.rsq), M);", "  if ((uint32_t)yRv[4 * i] & 1u) okv[i] = 1;\n"),
}


def test_the_analysis_refuses_a_planted_branch_on_a_secret_bit(tmp_path):
    """The mutations, in the source: one `if` on a bit of k0, one on the parity of y(R), each compiled here from a copy.  The analysis has to refuse the mutated
    kernel; the shipped source compiled by the same command passes, and so does the kernel a mutation did not touch."""
    src = open(os.path.join(CSRC, "k_schnorr.hip")).read()
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    texts = {"shipped": src}
    for name, (_, _, anchor, plant) in PLANTS.items():
        assert src.count(anchor) == 1, name
        texts[name] = src.replace(anchor, plant + anchor)
    for name, text in texts.items():
        unit, out = tmp_path / f"{name}.hip", tmp_path / f"{name}.s"
        unit.write_text(text)
        subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=900)
        asm = out.read_text()
        for kernel, secrets in ((NONCE, NONCE_SECRETS), (FINISH, FINISH_SECRETS)):
            if name != "shipped" and PLANTS[name][0] == kernel:
                with pytest.raises(ct_check.Violation) as exc:
                    ct_check.check_secret_flow(asm, kernel, secret_args=secrets)
                assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
            else:
                ct_check.check_secret_flow(asm, kernel, secret_args=secrets)
