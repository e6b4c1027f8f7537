"""Deterministic ECDSA signing, the part that needs no GPU: the three entry points are declared, exported and callable from C99; the host model the GPU tests
take their expected values from (tools/rfc6979_model.py) gives the known answers of RFC 6979 A.2.5 and rejects candidates at the odds the curves' orders
predict; C(n) is the table's; the new kernels exist in the shipped gfx950 listing without scratch memory; the nonce kernels keep d, the HMAC state, the
candidates and the nonce out of every branch condition and address (tools/ct_check.py check_secret_flow) with the retry byte as the one public value, and
the analysis refuses a planted branch on another bit of the candidate."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                # noqa: E402
import rfc6979_model as model  # noqa: E402
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_mul  # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
NEW_SYMBOLS = ("ecsimd_hip_sha256", "ecsimd_hip_rfc6979_nonce", "ecsimd_hip_ecdsa_sign_deterministic")
NEW_KERNELS = ("8k_sha256E", "15k_rfc6979_first", "15k_rfc6979_retry")
# scalar memory writes and what goes with them are off limits on the machines this runs on, in any letter case, comments and strings included -- which is
# why the words are put together here instead of being written out
FORBIDDEN = re.compile("|".join("s_" + w for w in ("store_" + "dword", "buffer_" + "store", "scratch_" + "store", "atomic_", "buffer_" + "atomic", "dcache_" + "wb", "dcache_" + "discard")), re.I)
# k_rfc6979_first(order, e, d, k, state, retry, ok, n): order is 32 bytes BY VALUE, one argument.  Secret: d, the nonce / candidate buffer, the K / V state.
FIRST, FIRST_SECRETS, FIRST_RETRY = "k_rfc6979_first", [2, 3, 4], 5
# k_rfc6979_retry(order, k, state, retry, ok, n, cap)
RETRY, RETRY_SECRETS, RETRY_RETRY = "k_rfc6979_retry", [1, 2], 3


def curve_dicts():
    from ecsimd_amd.curves import NAMED
    return {"p256": CURVE_PARAMS[P256], "secp256k1": CURVE_PARAMS[SECP256K1], **NAMED}


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def sha_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_sha256-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, "k_sha256.hip")), listing
    return open(listing).read()


# ---- the C ABI
def test_the_three_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
    header = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    assert "this library has no hash" not in header
    from ecsimd_amd import Engine
    for m in ("sha256", "rfc6979_nonce", "ecdsa_sign_deterministic"):
        assert callable(getattr(Engine, m))


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_sha256(NULL, b, 32, 32, w, 0);
    rc |= ecsimd_hip_rfc6979_nonce(NULL, ECSIMD_HIP_SECP256K1, w, w, w, b, 0);
    rc |= ecsimd_hip_ecdsa_sign_deterministic(NULL, ECSIMD_HIP_P256, w, w, w, w, NULL, b, 0, ECSIMD_HIP_ECDSA_LOW_S);
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
    """RFC 6979 A.2.5 (P-256, SHA-256): k, r and s of "sample" and "test" (tests/golden/rfc6979_p256_sha256.json)."""
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "rfc6979_p256_sha256.json")))
    c = CURVE_PARAMS[P256]
    d = int(kat["d"], 16)
    assert ec_mul(P256, d, (c["gx"], c["gy"])) == (int(kat["qx"], 16), int(kat["qy"], 16))
    assert len(kat["cases"]) == 2
    for case in kat["cases"]:
        e = model.digest_int(case["message"].encode())
        k, rejected = model.nonce(c["n"], e, d)
        assert (k, rejected) == (int(case["k"], 16), 0)
        r, s, v, k2 = model.sign(c, e, d)
        assert (r, s, k2) == (int(case["r"], 16), int(case["s"], 16), k) and v in (0, 1)
        kG = ec_mul(P256, k, (c["gx"], c["gy"]))                                  # the textbook signature with that nonce
        assert r == kG[0] % c["n"] and s == pow(k, -1, c["n"]) * (e + r * d) % c["n"]
    assert {case["message"] for case in kat["cases"]} == {"sample", "test"}


def test_the_model_refuses_keys_out_of_range_and_reduces_the_digest():
    for name, c in curve_dicts().items():
        n = c["n"]
        for d in (0, n, n + 1, 2**256 - 1):
            assert model.nonce(n, 12345, d) is None and model.sign(c, 12345, d) is None
        assert model.nonce(n, n + 5, 77) == model.nonce(n, 5, 77) != model.nonce(n, 6, 77)          # bits2octets: e - n where e >= n
        assert model.nonce(n, n, 77) == model.nonce(n, 0, 77)
        assert model.nonce(n, 2**256 - 1, 1)[0] in range(1, n)
    with pytest.raises(ValueError):
        model.nonce(2**255 - 19, 1, 1)                                                               # qlen = 256 only


@pytest.mark.parametrize("name, lanes_expected, sigmas", [("brainpoolP256r1", 0.336, 4), ("frp256v1", 0.055, 4)])
def test_rejections_follow_the_orders_odds(name, lanes_expected, sigmas):
    """Over 4 096 random (e, d): the lanes with at least one rejection are binomial with the curve's odds 1 - n / 2^256."""
    n = curve_dicts()[name]["n"]
    odds = 1 - n / 2**256
    assert abs(odds - lanes_expected) < 1e-3
    rng = random.Random(name)
    lanes = 4096
    rejected = [model.nonce(n, rng.getrandbits(256), rng.randrange(1, n))[1] for _ in range(lanes)]
    hit = sum(1 for x in rejected if x)
    assert abs(hit - lanes * odds) < sigmas * (lanes * odds * (1 - odds)) ** 0.5, hit
    if name == "brainpoolP256r1":
        assert hit >= lanes // 4 and max(rejected) >= 3
        total = sum(rejected)                                                                     # candidates rejected in all: geometric, mean odds / (1 - odds) per lane
        assert abs(total - lanes * odds / (1 - odds)) < 0.1 * lanes * odds / (1 - odds)
    assert model.nonce(n, 1, 1, cap=1) is None or model.nonce(n, 1, 1)[1] == 0                    # a cap of one candidate refuses exactly the lanes that would retry
    retrying = next(i for i in range(10**6) if model.nonce(n, i, 1)[1] >= 1)
    assert model.nonce(n, retrying, 1, cap=1) is None and model.nonce(n, retrying, 1, cap=model.nonce(n, retrying, 1)[1] + 1) == model.nonce(n, retrying, 1)


def test_candidates_needed_is_the_table():
    want = {"secp256k1": 2, "p256": 4, "sm2": 4, "frp256v1": 31, "brainpoolP256r1": 82}
    assert {name: model.candidates_needed(c["n"]) for name, c in curve_dicts().items()} == want
    for name, c in curve_dicts().items():                                                          # the definition, on exact integers
        miss, C = 2**256 - c["n"], want[name]
        assert miss ** (C - 1) << 128 > 2 ** (256 * (C - 1))                                       # one candidate fewer does not reach 2^-128 ...
        assert (miss ** C << 128) << 90 <= (2 ** (256 * C)) * (2**90 + 1)                               # ... C do (SM2: to within the rounding of its quotient to 2^-32)
    assert model.candidates_needed(2**255) == 128                                                  # the smallest order supported: never more than 128 candidates


# ---- the shipped ISA
def test_new_kernels_exist_and_use_no_scratch(sha_asm):
    meta = sha_asm[sha_asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    for k in NEW_KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", hit[0]), k
    assert "scratch_" not in sha_asm
    assert "k_sha256.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_compression_is_register_resident_and_uses_the_bit_instructions(sha_asm):
    """One compression is ~1 500 VALU instructions: rotations as v_alignbit_b32, Ch and Maj as one three-input bit operation each (v_bitop3_b32 on gfx950,
    the successor of v_bfi_b32).  k_rfc6979_first holds 9 compressions in its text (7 in the loop over steps d-g, 2 for the candidate)."""
    body = "\n".join(i for _, _, insts in ct_check.parse_function(sha_asm, FIRST) for i in insts)
    valu = len(re.findall(r"^v_", body, re.M))
    assert 9 * 1200 < valu < 9 * 2000, valu
    assert len(re.findall(r"^v_alignbit_b32", body, re.M)) >= 9 * 64 * 6                          # 6 rotations per round at the very least
    assert len(re.findall(r"^v_(bitop3|bfi)_b32", body, re.M)) >= 9 * 64 * 2                      # Ch and Maj
    assert not re.search(r"^(ds_|buffer_|flat_)", body, re.M)


def test_no_off_limits_instruction_word_anywhere(sha_asm):
    assert not FORBIDDEN.search(sha_asm)
    for f in ("k_sha256.hip", "sha256.cuh", "capi.hip", "kernels.h"):
        assert not FORBIDDEN.search(open(os.path.join(CSRC, f)).read()), f


def test_nonce_kernels_keep_the_secrets_out_of_control_flow_and_addresses(sha_asm):
    rep = ct_check.check_secret_flow(sha_asm, FIRST, secret_args=FIRST_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]     # d: two 16-byte loads
    assert rep["public_branches"] >= 1
    rep = ct_check.check_secret_flow(sha_asm, RETRY, secret_args=RETRY_SECRETS)
    assert rep["secret_loads"] >= 6 and not rep["secret_scratch"] and not rep["secret_lds"]     # K's two midstates and V: six 16-byte loads
    assert rep["public_branches"] >= 2                                                           # the batch's tail, and the loop over the reloaded retry byte
    # the declassification is the naming of ONE buffer: with `retry` secret as well, the loop's branch is a violation
    with pytest.raises(ct_check.Violation):
        ct_check.check_secret_flow(sha_asm, RETRY, secret_args=RETRY_SECRETS + [RETRY_RETRY])
    # SHA-256 by itself handles public data; named secret, its message would still reach no branch and no address (one instruction stream per length)
    assert ct_check.check_secret_flow(sha_asm, "k_sha256E", secret_args=[0])["secret_loads"] >= 1


def test_the_analysis_refuses_a_branch_on_another_bit_of_the_candidate(tmp_path):
    """The mutation, in the source: k_rfc6979_retry with one `if` added -- leave the loop where bit 0 of the candidate is set -- compiled here.  The analysis has to refuse it; the shipped
    source compiled by the same command passes."""
    src = open(os.path.join(CSRC, "k_sha256.hip")).read()
    anchor = "    candidate_out(V, N, 0xffffffffu, kv, again, okv, i);\n"
    assert src.count(anchor) == 1
    planted = src.replace(anchor, "    if (V.h[7] & 1u) break;\n" + anchor)
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    for name, text, refused in (("shipped", src, False), ("planted", planted, True)):
        unit, out = tmp_path / f"{name}.hip", tmp_path / f"{name}.s"
        unit.write_text(text)
        subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=900)
        asm = out.read_text()
        if refused:
            with pytest.raises(ct_check.Violation) as exc:
                ct_check.check_secret_flow(asm, RETRY, secret_args=RETRY_SECRETS)
            assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
            ct_check.check_secret_flow(asm, FIRST, secret_args=FIRST_SECRETS)                      # the kernel that was not touched still passes
        else:
            ct_check.check_secret_flow(asm, RETRY, secret_args=RETRY_SECRETS)
