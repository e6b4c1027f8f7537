"""Ed25519, the part that needs no GPU: the entry points are declared in a header of their own, exported beside (not among) the ecsimd_hip_* set, and callable
from C99; the host model the GPU tests take their expected values from (tools/ed25519_model.py) gives the fixture bit for bit, rejects every one-bit change
of each known answer and the rule set's edge encodings, and agrees with libcrypto where libcrypto loads; tests/golden/ed25519_verdicts.json (refused and
accepted lanes of every kind, keys and R with a small-order component among them) is reproduced by the model and by libcrypto, record for record; the new kernels exist in the shipped gfx950 listing,
the secret ones without scratch memory or LDS; those keep the seed, a, r and the products out of every branch condition, address and lane mask
(tools/ct_check.py check_secret_flow), and the analysis refuses a planted branch on one bit of a; the host functions wipe through wipe_workspace over their
own carve's total."""
import hashlib
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as model   # noqa: E402
import capi_ed25519_shape       # noqa: E402
import capi_secret_shape        # noqa: E402
import ct_check                 # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_ed25519.h")
NEW_SYMBOLS = ("ecsimd_ed25519_pubkey", "ecsimd_ed25519_sign", "ecsimd_ed25519_verify", "ecsimd_ed25519_raw")
NEW_KERNELS = ("k_ed_secret_frontILb0E", "k_ed_secret_frontILb1E", "12k_ed_base_ct", "16k_ed_sign_finish", "17k_ed_verify_front", "16k_ed_verify_loop", "8k_ed_raw")
SECRET_KERNELS = NEW_KERNELS[:4]
# k_ed_secret_front(gmod BY VALUE, seed, seed_aligned, msg, msg_bytes, stride, lens, aligned, a, r, n): the seed and the workspace arrays a and r
FRONT, FRONT_SECRETS = "k_ed_secret_frontILb1E", [1, 8, 9]
FRONT_PUBKEY = "k_ed_secret_frontILb0E"
# k_ed_base_ct(k, out, out_aligned, n): the scalar (a, then r) and the product's encoding (public once returned, secret until then)
COMB, COMB_SECRETS = "k_ed_base_ct", [0, 1]
# k_ed_sign_finish(gmod, a, r, encA, encR, msg, msg_bytes, stride, lens, aligned, sig, sig_aligned, pk, pk_aligned, n): a, r and both products
FINISH, FINISH_SECRETS = "k_ed_sign_finish", [1, 2, 3, 4]
P, L = model.P, model.L


def le32(v):
    return int(v).to_bytes(32, "little")


def fixture():
    return [(bytes.fromhex(c["seed"]), bytes.fromhex(c["message"]), bytes.fromhex(c["public_key"]), bytes.fromhex(c["signature"]), c["source"])
            for c in json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json")))["cases"]]


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def ed_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_ed25519.hip", "ed25519.cuh", "fe25519.cuh", "ed25519_base.inc"):
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    return open(listing).read()


# ---- the C ABI
def test_the_four_functions_are_declared_in_their_own_header_and_exported(built):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_ed25519_[a-z0-9_]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(built, s), s
    assert '#include "ecsimd_hip.h"' in text and "ECSIMD_ED25519_REJECT_SMALL_ORDER = 1" in text
    assert "25519" not in open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()                 # nothing was added to the other header
    import ecsimd_amd
    from ecsimd_amd import Engine
    for m in ("ed25519_pubkey", "ed25519_sign", "ed25519_verify", "ed25519_raw"):
        assert callable(getattr(Engine, m)), m
    assert ecsimd_amd.ED25519_REJECT_SMALL_ORDER == 1 and "ED25519_REJECT_SMALL_ORDER" in ecsimd_amd.__all__


def test_the_ecsimd_hip_exports_are_still_exactly_the_declared_set(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_hip_")} == set(declared_symbols())
    declared = set(re.findall(r"\b(ecsimd_ed25519_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    assert {s for s in exported if s.startswith("ecsimd_ed25519_")} == declared


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_ed25519.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint8_t* b = NULL; const uint32_t* lens = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_ed25519_pubkey(NULL, b, b, 0);
    rc |= ecsimd_ed25519_sign(NULL, b, b, 3, 8, lens, b, NULL, 0);
    rc |= ecsimd_ed25519_verify(NULL, b, b, 3, 8, lens, b, b, 0, ECSIMD_ED25519_REJECT_SMALL_ORDER);
    rc |= ecsimd_ed25519_raw(NULL, ECSIMD_ED25519_RAW_FE_MUL, b, b, 0);
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
def test_the_model_gives_the_fixture_bit_for_bit():
    fx = fixture()
    assert len(fx) >= 30 and sum(c[4].startswith("RFC 8032") for c in fx) == 3
    assert {len(c[1]) for c in fx} >= {0, 1, 2, 79, 80, 81, 95, 96, 97, 128, 207, 208, 300}
    for seed, msg, pk, sig, _ in fx:
        assert model.pubkey(seed) == pk
        assert model.sign(seed, msg) == (sig, pk)
        assert model.verify(pk, msg, sig) and model.verify(pk, msg, sig, True)
    assert fx[0][2].hex().startswith("d75a9801") and fx[0][3].hex().startswith("e5564300") and fx[0][3].hex().endswith("100b")       # RFC 8032 7.1 TEST 1
    assert fx[1][2].hex().startswith("3d4017c3") and fx[2][2].hex().startswith("fc51cd8e")
    assert model.table_text() == open(os.path.join(CSRC, "ed25519_base.inc")).read()                 # the device constants are the model's


def test_the_model_rejects_every_one_bit_change():
    for seed, msg, pk, sig, _ in fixture()[:6]:
        for bit in range(256):
            flip = lambda b: (int.from_bytes(b, "little") ^ (1 << bit)).to_bytes(32, "little")
            assert not model.verify(flip(pk), msg, sig), bit
            assert not model.verify(pk, msg, flip(sig[:32]) + sig[32:]), bit
            assert not model.verify(pk, msg, sig[:32] + flip(sig[32:])), bit
        for bit in range(8 * len(msg)):
            m2 = bytearray(msg); m2[bit >> 3] ^= 1 << (bit & 7)
            assert not model.verify(pk, bytes(m2), sig), bit
        assert not model.verify(pk, msg + b"\x00", sig) and (not msg or not model.verify(pk, msg[:-1], sig))


def test_the_model_agrees_with_libcrypto():
    ossl = model.libcrypto()
    if ossl is None:
        return                                                                                        # (the comparison exists only where libcrypto loads)
    rng = random.Random(1087)
    for j in range(60):
        seed, msg = rng.randbytes(32), rng.randbytes(rng.choice((0, 1, 31, 32, 47, 48, 64, 111, 112, 200)))
        sig, pk = model.sign(seed, msg)
        assert (sig, pk) == ossl.sign(seed, msg)
        assert model.verify(pk, msg, sig) and ossl.verify(pk, msg, sig)
        for what in range(4):                                                                         # one bit of pk, R, s, the message
            bit = rng.randrange(256 if what < 2 else 252 if what == 2 else max(1, 8 * len(msg)))
            flip = lambda b: (int.from_bytes(b, "little") ^ (1 << bit)).to_bytes(len(b), "little")
            if what == 3 and not msg:
                continue
            case = ((flip(pk), msg, sig) if what == 0 else (pk, msg, flip(sig[:32]) + sig[32:]) if what == 1 else (pk, msg, sig[:32] + flip(sig[32:])) if what == 2
                    else (pk, flip(msg), sig))
            assert model.verify(*case) == ossl.verify(*case) == False, (j, what)                      # noqa: E712
        s = int.from_bytes(sig[32:], "little")
        if s + L < 2**256:
            assert not model.verify(pk, msg, sig[:32] + le32(s + L)) and not ossl.verify(pk, msg, sig[:32] + le32(s + L))
    # the stated difference: libcrypto accepts these non-canonical A, this rule set refuses them
    for enc in (le32(P + 1), le32(1 | (1 << 255))):
        sig = le32(1) + le32(0)                                                                      # R = identity, s = 0 under A = "identity"
        assert not model.verify(enc, b"", sig)
        assert ossl.verify(enc, b"", sig), "libcrypto no longer accepts this non-canonical A: the header's note is out of date"


def test_the_model_refuses_the_edge_encodings():
    ident, zero = le32(1), le32(0)
    for i in range(19):
        assert model.decode(le32(P + i)) is None and not model.verify(le32(P + i), b"", ident + zero), i      # y = p .. p + 18
    assert model.decode(le32(P - 1)) is not None                                                               # ... and p - 1 is a point (order 2)
    assert model.decode(le32(1 | (1 << 255))) is None and model.decode(le32((P - 1) | (1 << 255))) is None     # x = 0 with the sign bit set
    assert model.decode(le32(2)) is None and not model.verify(le32(2), b"", ident + zero)                      # y = 2: no point
    assert model.verify(ident, b"any message", ident + zero)                                                   # A = identity, R = identity, s = 0: the equation holds
    assert not model.verify(ident, b"any message", ident + zero, reject_small_order=True)
    assert not model.verify(ident, b"", le32(P + 1) + zero)                                                    # a non-canonical R never equals a canonical encoding
    assert len(set(model.SMALL_ORDER)) == 8
    for e in model.SMALL_ORDER:
        pt = model.decode(e)
        assert pt is not None and model.encode(pt) == e and model.pt_eq(model.pt_mul(8, pt), model.IDENTITY)
    assert model.sc_reduce(le32(L) + bytes(32)) == 0 and model.base_mult(L) == ident and model.base_mult(1) == le32(model.BY)
    assert model.expand(bytes(32))[0] % 8 == 0 and model.expand(bytes(32))[0] >> 254 == 1


# ---- the verdict fixture
def verdict_records():
    return json.load(open(model.VERDICTS_PATH))["records"]


def test_the_model_reproduces_every_verdict_of_the_fixture():
    recs = verdict_records()
    golden = os.path.dirname(model.VERDICTS_PATH)
    assert 1000 <= len(recs) <= 1500                                                                  # one batch on the device
    assert os.path.getsize(model.VERDICTS_PATH) < max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(model.VERDICTS_PATH))
    for r in recs:
        pk, msg, sig = bytes.fromhex(r["public_key"]), bytes.fromhex(r["message"]), bytes.fromhex(r["signature"])
        assert len(msg) <= 16 and len(pk) == 32 and len(sig) == 64
        assert int(model.verify(pk, msg, sig)) == r["model"], r
        assert int(model.verify(pk, msg, sig, True)) == r["model_strict"], r


def test_libcrypto_reproduces_every_verdict_of_the_fixture():
    ossl = model.libcrypto()
    if ossl is None:
        return                                                                                        # (the comparison exists only where libcrypto loads)
    for r in verdict_records():
        assert int(ossl.verify(bytes.fromhex(r["public_key"]), bytes.fromhex(r["message"]), bytes.fromhex(r["signature"]))) == r["libcrypto"], r


def test_the_fixtures_classes_divergences_and_mixed_order_predicate():
    recs = verdict_records()
    kinds = model.check_verdicts(recs)                                                                # model == libcrypto off the divergent kind, both verdicts per class
    divergent = [r for r in recs if r.get("divergent")]
    assert [r["kind"] for r in divergent] == [model.DIVERGENT_KIND] * 2 == [r["kind"] for r in recs if r["kind"] == model.DIVERGENT_KIND]
    assert all((r["libcrypto"], r["model"], r["model_strict"]) == (1, 0, 0) for r in divergent)       # the header's stated difference, and nothing else
    assert all(r["libcrypto"] == r["model"] for r in recs if not r.get("divergent"))
    assert kinds["small order"] == 512 and sum(r["model"] for r in recs if r["kind"] == "small order") == 60
    # the classes (order of t_a, order of t_r), counted here without check_verdicts: accepted and refused
    count = {}
    for r in recs:
        if r["kind"] in model.MIXED_KINDS:
            count.setdefault(tuple(r["orders"]), [0, 0])[r["model"]] += 1
            assert r["model"] == r["holds"] == r["libcrypto"] == r["model_strict"], r
    assert set(count) == {(a, b) for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)} - {(1, 1)}
    for (a, b), (refused, accepted) in count.items():
        assert refused >= 8 and (accepted >= 8 if a % b == 0 else accepted == 0), (a, b, refused, accepted)
    # the predicate from the parts, on torsion points alone: t_r + [h]t_a = O has a solution exactly where the order of t_r divides that of t_a
    tors = model.torsion()
    assert [n for _, _, n in tors] == [1, 2, 4, 4, 8, 8, 8, 8]
    for _, ta, na in tors:
        for _, tr, nr in tors:
            assert any(model.pt_eq(model.pt_add(tr, model.pt_mul(h, ta)), model.IDENTITY) for h in range(8)) == (na % nr == 0)
    # a mixed-order key is no small-order encoding, decodes, and has order 8 L at most: [L]A is the torsion part times L mod 8 = 5
    rng = random.Random(8)
    for _, t, n in tors[1:]:
        a = rng.randrange(1, L)
        pt = model.mixed(model.base_point_mul(a), t)
        enc = model.encode(pt)
        assert enc not in model.SMALL_ORDER and model.pt_eq(model.decode(enc), pt)
        assert model.pt_eq(model.pt_mul(L, pt), model.pt_mul(5, t)) and not model.pt_eq(model.pt_mul(L, pt), model.IDENTITY)
        assert model.pt_eq(model.pt_mul(8 * L, pt), model.IDENTITY)


def test_sign_mixed_states_the_verdict_the_model_and_libcrypto_reach():
    ossl = model.libcrypto()
    tors = model.torsion()
    rng = random.Random(2280)
    seen = set()
    for j in range(48):
        (_, ta, na), (_, tr, nr) = tors[rng.randrange(8)], tors[rng.randrange(8)]
        pk, sig, holds = model.sign_mixed(rng.randrange(1, L), rng.randrange(1, L), ta, tr, b"%d" % j)
        assert model.verify(pk, b"%d" % j, sig) == holds and (ossl is None or ossl.verify(pk, b"%d" % j, sig) == holds), (j, na, nr)
        seen.add(holds)
    assert seen == {True, False}


def test_the_small_order_words_in_the_device_source_are_the_models():
    src = open(os.path.join(CSRC, "k_ed25519.hip")).read()
    table = re.search(r"S\[3\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [b"".join(int(x, 16).to_bytes(4, "little") for x in re.findall(r"0x([0-9a-fA-F]{8})u", row)) for row in re.findall(r"\{([^{}]*)\}", table)]
    assert rows == [model.SMALL_ORDER[1], model.SMALL_ORDER[4], model.SMALL_ORDER[6]]


# ---- the shipped ISA
def kernel_blocks(asm):
    meta = asm[asm.index(".amdgpu_metadata"):]
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}


def test_every_new_kernel_is_in_the_listing_and_the_secret_ones_use_no_scratch(ed_asm):
    blocks = kernel_blocks(ed_asm)
    assert len(blocks) == len(NEW_KERNELS), sorted(blocks)
    for k in NEW_KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        if k in SECRET_KERNELS:
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k
            assert re.search(r"\.vgpr_spill_count:\s+0\b", hit[0]), k
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", hit[0]), k                       # no LDS either: nothing would wipe it
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_ed25519.hip", "fe25519.cuh", "ed25519.cuh", "ed25519_base.inc"):
        assert f in makefile, f


def test_the_secret_kernels_keep_the_secrets_out_of_control_flow_and_addresses(ed_asm):
    rep = ct_check.check_secret_flow(ed_asm, FRONT, secret_args=FRONT_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]          # the seed: 32 bytes
    assert rep["public_branches"] >= 2                                                               # the batch's tail, the block loop, the words of the message
    rep = ct_check.check_secret_flow(ed_asm, FRONT_PUBKEY, secret_args=FRONT_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]
    rep = ct_check.check_secret_flow(ed_asm, COMB, secret_args=COMB_SECRETS)
    assert rep["secret_loads"] == 2 and not rep["secret_scratch"] and not rep["secret_lds"]          # the scalar: two 16-byte loads; the table is read at public addresses
    rep = ct_check.check_secret_flow(ed_asm, FINISH, secret_args=FINISH_SECRETS)
    assert rep["secret_loads"] >= 8 and not rep["secret_scratch"] and not rep["secret_lds"]          # a, r and both encodings
    # with the MESSAGE named secret as well nothing changes: its bytes reach no branch and no address (lengths and strides are the call's)
    ct_check.check_secret_flow(ed_asm, FRONT, secret_args=FRONT_SECRETS + [3])
    ct_check.check_secret_flow(ed_asm, FINISH, secret_args=FINISH_SECRETS + [5])


def test_the_comb_reads_every_entry_of_a_row(ed_asm):
    """The constant-time comb's table reads are scalar loads at addresses made of the row alone: 8 entries x 96 bytes = 768 bytes per selection, in the text of
    both loops; no vector load but the scalar's, no LDS."""
    body = "\n".join(i for _, _, insts in ct_check.parse_function(ed_asm, COMB) for i in insts)
    loads = re.findall(r"^s_load_dwordx(\d+)", body, re.M)
    assert sum(4 * int(w) for w in loads if int(w) >= 8) >= 2 * 768
    assert len(re.findall(r"^global_load", body, re.M)) == 2 and not re.search(r"^(ds_|buffer_|flat_)", body, re.M)


PLANT_ANCHOR = "  fe_store(av, i, ed_sc_reduce256(a, M));\n"
PLANT = "  if (a.w[3] & 4u) av[4 * i + 1] = 1;\n"


def test_the_analysis_refuses_a_planted_branch_on_one_bit_of_a(tmp_path):
    src = open(os.path.join(CSRC, "k_ed25519.hip")).read()
    assert src.count(PLANT_ANCHOR) == 1
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    unit, out = tmp_path / "planted.hip", tmp_path / "planted.s"
    unit.write_text(src.replace(PLANT_ANCHOR, PLANT_ANCHOR + PLANT))
    subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=1200)
    asm = out.read_text()
    for kernel in (FRONT, FRONT_PUBKEY):
        with pytest.raises(ct_check.Violation) as exc:
            ct_check.check_secret_flow(asm, kernel, secret_args=FRONT_SECRETS)
        assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
    ct_check.check_secret_flow(asm, COMB, secret_args=COMB_SECRETS)                                   # the kernels the mutation did not touch still pass
    ct_check.check_secret_flow(asm, FINISH, secret_args=FINISH_SECRETS)


# ---- the host layer
def test_the_host_functions_wipe_through_wipe_workspace_over_their_own_carve(built):
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                                                      # still one wipe of the block and one user of the other comb's table
    body = capi_ed25519_shape.check_ed25519_secret_entry(src, "int ecsimd_ed25519_pubkey(", sign=False)
    assert "ed25519_secret_plan(ctx->workspace, chunk, false)" in body
    body = capi_ed25519_shape.check_ed25519_secret_entry(src, "int ecsimd_ed25519_sign(", sign=True)
    assert "ed25519_secret_plan(ctx->workspace, chunk, true)" in body
    verify = capi_secret_shape.function(src, "int ecsimd_ed25519_verify(")
    assert "hipMemcpy" not in verify and "Synchronize" not in verify and "ensure_workspace(ctx, ed25519_verify_plan(nullptr, chunk).bytes)" in verify
    for head in ("int ecsimd_ed25519_pubkey(", "int ecsimd_ed25519_sign(", "int ecsimd_ed25519_verify(", "int ecsimd_ed25519_raw("):
        assert "NO_COMPAT" not in capi_secret_shape.function(src, head) and "refuse_compat" not in capi_secret_shape.function(src, head), head   # compat contexts are accepted
    assert hashlib.sha512(b"").hexdigest().startswith("cf83e135")                                    # (hashlib's SHA-512 is what the model hashes with)
