"""The SM2 signature scheme, the part that needs no GPU: the entry points are declared in a header of their own, exported beside (not among) the ecsimd_hip_*
set, and callable from C99; the host model the GPU tests take their expected values from (tools/sm2_model.py) has an SM3 that equals hashlib's where hashlib
has one and the known answers everywhere, reproduces the standard's signature example and the fixture bit for bit, agrees with libcrypto where libcrypto
loads, and refuses every one-bit change of a valid (Q, e, r, s); sm3.cuh, compiled for the HOST, equals the model on the boundary lengths and Python
integers on the edge scalars; the new kernels exist once each in the shipped gfx950 listing, the secret ones without scratch memory or LDS, and keep their
secrets out of every branch condition, address and lane mask (tools/ct_check.py check_secret_flow), which refuses a branch planted on one bit of d; the host
functions wipe the workspace through the shared step over their own carve."""
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
import sm2_model as model       # noqa: E402
import capi_secret_shape        # noqa: E402
import ct_check                 # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_sm2.h")
SYMBOLS = {"ecsimd_sm2_curve", "ecsimd_sm2_sm3", "ecsimd_sm2_za", "ecsimd_sm2_digest", "ecsimd_sm2_pubkey", "ecsimd_sm2_verify_digest", "ecsimd_sm2_verify", "ecsimd_sm2_sign_digest"}
KERNELS = ("5k_sm3", "8k_sm2_za", "12k_sm2_digest", "20k_sm2_verify_scalars", "12k_sm2_accept", "18k_sm2_sign_scalars", "15k_sm2_key_range")
# the pointer arguments whose contents are secret, by position (argument 0 is the order's gmod, by value):
#   k_sm2_sign_scalars(M, e, d, k, x, r, s, ok, n, lanes, m)      d, k, x(k G), and what is made of them: r, s (which carries the prefix products), ok
#   k_sm2_key_range(M, d, qx, qy, ok, n)                           d, d G, the flag made of d
SECRET = {"k_sm2_sign_scalars": [2, 3, 4, 5, 6, 7], "k_sm2_key_range": [1, 2, 3, 4]}
P, N = model.P, model.N
ALL = 2**256 - 1
h64 = model.h64


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=3000)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def s_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_sm2-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_sm2.hip", "sm3.cuh", "gfield.cuh"):
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    return open(listing).read()


# ---- the C ABI
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_sm2_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_sm2")} == declared
    assert {s for s in exported if s.startswith("ecsimd_hip_")} == set(declared_symbols())       # still exactly the declared set
    assert '#include "ecsimd_hip.h"' in text
    other = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read().lower()
    assert "ecsimd_sm2" not in other and "sm3" not in other                                      # nothing was added to the other header
    from ecsimd_amd import Engine
    for m in ("sm2_curve", "sm3", "sm2_za", "sm2_digest", "sm2_pubkey", "sm2_verify_digest", "sm2_verify", "sm2_sign_digest", "sm2_sign"):
        assert callable(getattr(Engine, m)), m
    assert Engine.SM2_DEFAULT_ID == b"1234567812345678" == model.DEFAULT_ID


def test_the_curve_is_registered_once_and_is_the_named_one(built):
    import ctypes as C
    from ecsimd_amd import Engine, curves
    a, b = C.c_int(-1), C.c_int(-1)
    assert built.ecsimd_sm2_curve(C.byref(a)) == 0 and built.ecsimd_sm2_curve(C.byref(b)) == 0 and a.value == b.value >= 2
    assert built.ecsimd_sm2_curve(None) != 0
    assert Engine.sm2_curve() == a.value == curves.curve_id("sm2")
    c = curves.NAMED["sm2"]
    assert (c["p"], c["a"], c["b"], c["gx"], c["gy"], c["n"]) == (model.P, model.A, model.B, model.GX, model.GY, model.N)
    caps = C.c_int(0)
    assert built.ecsimd_hip_curve_capabilities(a, C.byref(caps)) == 0 and caps.value & 4                # ECSIMD_HIP_CURVE_ECDSA
    assert "#define ECSIMD_HIP_CURVE_ECDSA 4" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()) or \
        re.search(r"ECSIMD_HIP_CURVE_ECDSA\s*=\s*4\b", open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read())


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "sm2_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s


# ---- the model
def test_the_models_sm3_is_hashlibs_where_there_is_one_and_matches_the_known_answers():
    assert model.sm3(b"abc").hex() == "66c7f0f462eeedd9d1f2d46bdc10e4e24167c4875cf2f7a2297da02b8f4ba8e0" == model.SM3_ABC
    assert model.sm3(b"abcd" * 16).hex() == "debe9ff92275b8a138604889c18e5a4d6fdb70e5387e5765293dcba39c0c5732"        # GB/T 32905 appendix A.2
    assert model.sm3(b"").hex() == "1ab21d8355cfa17f8e61194831e81a8f22bec8c728fefb747ed035eb5082aa2b"
    try:
        hashlib.new("sm3")
    except ValueError:
        return                                                                                   # (the comparison exists only where hashlib has SM3)
    rng = random.Random(32905)
    for n in list(range(0, 130)) + [191, 192, 200, 255, 256, 1000]:
        m = bytes(rng.getrandbits(8) for _ in range(n))
        assert model.sm3(m) == hashlib.new("sm3", m).digest(), n


def test_the_model_reproduces_the_standards_example():
    ex = model.EXAMPLE
    q, ok = model.pubkey(ex["d"])
    assert ok == 1 and h64(q[0]).upper().startswith("09F9DF31") and model.on_curve(q)
    assert model.digest(q, ex["ident"], ex["msg"]) == ex["e"] == 0xF0B43E94BA45ACCAACE692ED534382EB17E6AB5A19CE7B31F4486FDFC0D28640
    assert model.sign(ex["ident"], ex["msg"], ex["d"], ex["k"]) == (ex["r"], ex["s"], 1)
    assert ex["r"] == 0xF5A03B0648D2C4630EEAC513E1BB81A15944DA3827D5B74143AC7EACEEE720B3 and ex["s"] == 0xB1B6AA29DF212FD8763182BC0D421CA1BB9038FD1F7F42D4840B69C485BBC1AA
    assert model.verify(q, ex["ident"], ex["msg"], ex["r"], ex["s"]) == 1
    assert model.mult(N) is None and model.on_curve(model.G) and model.high_x_point()[0] == N + 4 < P < 2 * N and 2**256 < 2 * N
    assert model.NONCE_CAP == 4


def test_the_model_reproduces_the_fixture_bit_for_bit():
    stored = json.load(open(model.FIXTURE))
    assert stored["adjudicated_by_libcrypto"] is True
    again = model.build_fixture(None)
    for key in ("curve", "nonce_candidates", "sm3", "example", "message", "digest", "sign"):
        assert again[key] == stored[key], key
    assert open(model.FIXTURE).read() == model.dump_fixture(stored)
    assert len(stored["message"]) >= 60 and {r["ok"] for r in stored["message"]} == {0, 1}
    ids, msgs = {len(r["id"]) // 2 for r in stored["message"]}, {len(r["msg"]) // 2 for r in stored["message"]}
    assert ids == set(model.ID_LENGTHS) == {0, 16, 53, 54, 61, 62, 100} and msgs == set(model.MSG_LENGTHS) == {0, 23, 24, 31, 32, 100}
    assert {(194 + i) % 64 for i in ids} >= {55, 56, 63, 0} and {(32 + m) % 64 for m in msgs} >= {55, 56, 63, 0}
    assert [len(r["msg"]) // 2 for r in stored["sm3"][2:]] == [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 200]
    notes = " | ".join(r["note"] for r in stored["digest"])
    for want in ("e >= n", "x(R) = n + 4", "r + s = n", "point at infinity", "r = 0", "r = n", "s = 0", "s = n", "off the curve", "p + ", "y >= p", "Q = (0, 0)"):
        assert want in notes, want
    assert [r["by"] for r in stored["digest"]].count("model") == 4 and all(r["ok"] == 0 for r in stored["digest"] if r["by"] == "model")
    notes = " | ".join(r["note"] for r in stored["sign"])
    for want in ("d = 1,", "d = n - 2", "d = n - 1", "d = 0", "d = n,", "k = 0", "k = n", "k = n - 1", "r + k = n", "deterministic"):
        assert want in notes, want
    ex = stored["example"]
    assert int(ex["e"], 16) == model.EXAMPLE["e"] and int(ex["r"], 16) == model.EXAMPLE["r"] and int(ex["s"], 16) == model.EXAMPLE["s"] and ex["qx"].startswith("09f9df31")
    for r in stored["sign"]:                                                                    # the rule set, record by record
        e, d, k = int(r["e"], 16), int(r["d"], 16), None if r["k"] is None else int(r["k"], 16)
        kk = model.nonce(e, d) if k is None else k
        want = int(1 <= d <= N - 2 and kk is not None and 1 <= kk <= N - 1)
        if want:
            rr = (e + model.mult(kk)[0]) % N
            want = int(rr != 0 and rr + kk != N and (pow(1 + d, -1, N) * (kk - rr * d)) % N != 0)
        assert r["ok"] == want and r["key_ok"] == int(1 <= d <= N - 2), r["note"]
        if r["ok"]:
            assert model.verify_digest((int(r["qx"], 16), int(r["qy"], 16)), e, int(r["r"], 16), int(r["s"], 16)) == 1, r["note"]


def test_the_model_agrees_with_libcrypto():
    adj = model.libcrypto()
    if adj is None:
        return                                                                                   # (the comparison exists only where libcrypto loads and knows SM2)
    fx = model.load_fixture()
    I = lambda r, k: int(r[k], 16)
    for r in fx["message"]:
        q, ident, msg = (I(r, "qx"), I(r, "qy")), bytes.fromhex(r["id"]), bytes.fromhex(r["msg"])
        if ident:
            assert adj.verify(q, ident, msg, I(r, "r"), I(r, "s")) == r["ok"], r["note"]
        else:                                                                                    # libcrypto's message interface takes no empty ID: the digest level decides
            assert adj.verify(q, ident, msg, I(r, "r"), I(r, "s")) == 0
            assert adj.verify_digest(q, model.digest(q, ident, msg), I(r, "r"), I(r, "s")) == r["ok"], r["note"]
    for r in fx["digest"]:
        got = adj.verify_digest((I(r, "qx"), I(r, "qy")), I(r, "e"), I(r, "r"), I(r, "s"))
        assert (got is None and r["by"] == "model") or (got == r["ok"] and r["by"] == "libcrypto"), r["note"]
    for r in fx["sign"]:
        if r["ok"]:
            assert adj.verify_digest((I(r, "qx"), I(r, "qy")), I(r, "e"), I(r, "r"), I(r, "s")) == 1, r["note"]
    assert model.build_fixture(adj)["digest"] == fx["digest"]                                    # every verdict asked again: an exception where the two differ


def test_every_one_bit_change_of_a_valid_signature_is_refused():
    ex = model.EXAMPLE
    q = model.mult(ex["d"])
    e, r, s = ex["e"], ex["r"], ex["s"]
    assert model.verify_digest(q, e, r, s) == 1
    for bit in range(256):
        f = 1 << bit
        assert model.verify_digest((q[0] ^ f, q[1]), e, r, s) == 0, ("qx", bit)
        assert model.verify_digest((q[0], q[1] ^ f), e, r, s) == 0, ("qy", bit)
        assert model.verify_digest(q, e ^ f, r, s) == 0, ("e", bit)
        assert model.verify_digest(q, e, r ^ f, s) == 0, ("r", bit)
        assert model.verify_digest(q, e, r, s ^ f) == 0, ("s", bit)


# ---- the device's hash and integer rules, compiled for the host
def test_sm3_the_walkers_the_z_a_stream_and_the_verification_rules_on_the_host(tmp_path):
    exe = tmp_path / "sm2_host_check"
    subprocess.run(["hipcc", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "sm2_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=1200)
    rng = random.Random(3)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    hx = lambda b: b.hex() if b else "-"
    reqs, exps = [], []

    def ask(line, exp):
        reqs.append(line); exps.append(list(exp))
    for n in sorted(set(model.SM3_LENGTHS) | set(range(0, 70)) | {118, 119, 120, 121, 127, 128, 129, 191, 192, 193, 200, 300}):
        m = rb(n)
        for aligned, off in ((1, 0), (1, 4), (0, 0), (0, 1), (0, 3)):
            ask("sm3 %d %d %s" % (aligned, off, hx(m)), [int(model.sm3(m).hex(), 16)])
    ask("sm3 1 0 " + hx(b"abc"), [int(model.SM3_ABC, 16)])
    ask("sm3 0 1 " + hx(b"abcd" * 16), [int(model.SM3_ABCD16, 16)])
    for n in sorted(set(model.MSG_LENGTHS) | set(range(0, 70)) | {87, 88, 95, 96, 100, 127, 128, 200}):
        z, m = rb(32), rb(n)
        for aligned, off in ((1, 0), (0, 1)):
            ask("after32 %d %d %s %s" % (aligned, off, z.hex(), hx(m)), [int(model.sm3(z + m).hex(), 16)])
    for n in sorted(set(model.ID_LENGTHS) | set(range(0, 70)) | {117, 118, 119, 125, 126, 127, 128, 129, 190, 1000, 8191}):
        ident, t = rb(n), rb(192)
        ask("za %s %s" % (hx(ident), t.hex()), [int(model.sm3((8 * n).to_bytes(2, "big") + ident + t).hex(), 16)])
    q = model.mult(model.EXAMPLE["d"])
    ask("za %s %s" % (model.DEFAULT_ID.hex(), b"".join(model.i2b(v) for v in (model.A, model.B, model.GX, model.GY, q[0], q[1])).hex()), [int(model.za(q).hex(), 16)])
    edge = [0, 1, 2, N - 2, N - 1, N, N + 1, P - 1, P, ALL, 2**255, 2**256 - N, N - 2**224] + [0xffffffff << (32 * j) for j in range(8)] + [rng.getrandbits(256) for _ in range(12)]
    for r in edge:
        for s in edge + [(N - r) % 2**256 if r <= N else 0]:
            valid = int(1 <= r < N and 1 <= s < N and (r + s) % N != 0)
            ask("vs %s %s %s" % (h64(r), h64(s), h64(N)), [valid, s * valid, (r + s) % N * valid])
    for e in edge:
        for x in edge[:14] + [rng.getrandbits(256)]:
            want = (e % N + x % N) % N
            ask("acc %s %s %s %s" % (h64(e), h64(x), h64(want), h64(N)), [1])
            ask("acc %s %s %s %s" % (h64(e), h64(x), h64(want ^ 1), h64(N)), [0])
            ask("acc %s %s %s %s" % (h64(e), h64(x), h64((want + N) % 2**256), h64(N)), [int((want + N) % 2**256 == want)])
    out = subprocess.run([str(exe)], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=600)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == len(reqs), out.stderr[-500:]
    wrong = [r[:90] for r, e, l in zip(reqs, exps, lines) if [int(x, 16) for x in l.split()] != e]
    assert not wrong, (len(wrong), wrong[:5])


def test_the_compression_is_written_without_an_indexed_array():
    src = open(os.path.join(CSRC, "sm3.cuh")).read()
    body = src[src.index("SM3_FN void sm3_compress("):src.index("// ---- message bytes")]
    assert "#pragma unroll\n  for (int j = 0; j < 64; ++j)" in body and "& 15]" in body                 # the schedule rolls over sixteen registers, fully unrolled
    assert "sm3_bfi(a ^ b, c, b)" in body and "sm3_bfi(e, f, g)" in body                                # FF / GG of rounds 16 - 63 as bit selects
    assert "field.cuh" not in src.split("#pragma once")[1].split("namespace")[0]                        # stands alone: the host check compiles this very file


# ---- the shipped ISA
def kernel_blocks(asm):
    meta = asm[asm.index(".amdgpu_metadata"):]
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}


def test_every_new_kernel_is_in_the_listing_once_and_none_uses_scratch(s_asm):
    blocks = kernel_blocks(s_asm)
    assert len(blocks) == len(KERNELS), sorted(blocks)
    for k in KERNELS:
        hit = [b for name, b in blocks.items() if "_GLOBAL__N_1" + k + "E" in name]
        assert len(hit) == 1, k
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k                       # no scratch memory anywhere: no indexed array, no spill
        if k.lstrip("0123456789") in SECRET:
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", hit[0]), k
            assert "scratch_" not in "\n".join(i for b in ct_check.parse_function(s_asm, k.lstrip("0123456789")) for i in b[2]), k
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_sm2.hip", "sm3.cuh", "ecsimd_sm2.h"):
        assert f in makefile, f
    for unit in ("k_gfield.hip", "k_gcurve.hip", "k_p384.hip"):                                  # the new kernels stay out of the units whose kernel counts are pinned
        assert "sm2" not in open(os.path.join(CSRC, unit)).read().lower() and "sm3" not in open(os.path.join(CSRC, unit)).read().lower(), unit
    import glob
    guard = re.search(r'glob\.glob\(os\.path\.join\(ROOT, "build", "csrc", "([^"]+)"\)\)', open(os.path.join(ROOT, "tests", "test_isa_guards.py")).read()).group(1)
    assert any(os.path.basename(f).startswith("k_sm2-") for f in glob.glob(os.path.join(ROOT, "build", "csrc", guard)))


def test_the_recorded_listing_figures_are_the_shipped_ones(s_asm):
    import sm2_listing
    recorded = json.load(open(os.path.join(ROOT, "profiles", "r20", "sm2_listing.json")))
    assert sm2_listing.report(s_asm) == recorded
    for k, row in recorded["kernels"].items():
        assert row["scratch_bytes"] == 0, k
    assert 500 < recorded["valu_per_compression"] < 2500


@pytest.mark.timeout(1200)
def test_the_secret_kernels_keep_the_secrets_out_of_control_flow_and_addresses(s_asm):
    for k, args in SECRET.items():
        rep = ct_check.check_secret_flow(s_asm, k, secret_args=args)
        assert rep["secret_loads"] >= 3 and not rep["secret_scratch"] and not rep["secret_lds"], (k, rep)
        assert rep["public_branches"] >= 1, (k, rep)                                             # the batch's tail (and the loops over a lane's elements)


def test_the_analysis_refuses_a_branch_planted_on_one_bit_of_d(s_asm):
    """In a COPY of the listing: behind the first load in k_sm2_key_range (d, or the point made of d), a compare of the loaded word and a branch on it."""
    start = s_asm.index("k_sm2_key_range")
    m = re.compile(r"\tglobal_load_dwordx4 v\[(\d+):\d+\], v\d+, s\[\d+:\d+\][^\n]*\n|\tglobal_load_dwordx4 v\[(\d+):\d+\], v\[\d+:\d+\], off[^\n]*\n").search(s_asm, start)
    reg = m.group(1) or m.group(2)
    label = re.compile(r"^(\.LBB\d+_\d+):", re.M).search(s_asm, m.end()).group(1)
    plant = "\ts_waitcnt vmcnt(0)\n\tv_and_b32_e32 v%s, 4, v%s\n\tv_cmp_ne_u32_e32 vcc, 0, v%s\n\ts_cbranch_vccnz %s\n" % (reg, reg, reg, label)
    planted = s_asm[:m.end()] + plant + s_asm[m.end():]
    with pytest.raises(ct_check.Violation) as exc:
        ct_check.check_secret_flow(planted, "k_sm2_key_range", secret_args=SECRET["k_sm2_key_range"])
    assert "condition" in str(exc.value) or "lane mask" in str(exc.value), exc.value
    ct_check.check_secret_flow(planted, "k_sm2_sign_scalars", secret_args=SECRET["k_sm2_sign_scalars"])      # a kernel the plant did not touch still passes


# ---- the host layer
def test_the_host_functions_wipe_through_the_shared_step_over_their_own_carve(built):
    src = capi_secret_shape.source()
    capi_secret_shape.check_shared_product(src)                                                  # still ONE wipe of the block in the whole file
    for head, plan, args, launches in (
            ("int ecsimd_sm2_sign_digest(", "sm2_sign_plan", ", n, k == nullptr", ["rfc6979_nonce", "sm2_sign_scalars"]),
            ("int ecsimd_sm2_pubkey(", "gc_plan", ", n", ["sm2_key_range"])):
        body = capi_secret_shape.function(src, head)
        assert re.findall(r"launch::(\w+)\(", body) == launches, head
        assert len(re.findall(r"\bsm2_secret_product\(", body)) == 1, head                       # the comb (or, under capture without a table, the ladder): one shared step
        assert "hipMemcpy" not in body and "Synchronize" not in body and "hipMemset" not in body, head        # nothing read back, no wipe of its own
        wipes = re.findall(r"^.*\bwipe_workspace\(.*$", body, re.M)
        assert len(wipes) == 1 and re.fullmatch(r"\s*const hipError_t err = wipe_workspace\(ctx, L\.bytes, hipGetLastError\(\)\);\s*", wipes[0]), (head, wipes)      # no `if` in front
        assert "ensure_workspace(ctx, %s(nullptr%s).bytes)" % (plan, args) in body and "L = %s(ctx->workspace%s);" % (plan, args) in body, head
        assert body.index("ensure_workspace(") < body.index("L = " + plan) < body.index("sm2_secret_product(") < body.index("launch::" + launches[-1]) < body.index("wipe_workspace("), head
        assert "launch::" not in body[body.index("wipe_workspace("):] and "return bad" not in body[body.index("L = " + plan):], head
        assert "at most 2^22" in body, head
    product = capi_secret_shape.function(src, "void sm2_secret_product(")
    assert "launch::gc_base_windowed_s(ctx->stream, rec.G, order_words(rec), 5, k, comb," in product and "hipMemcpy" not in product and "Synchronize" not in product
    planned = capi_secret_shape.function(src, "sm2_sign_layout sm2_sign_plan(")
    assert "gc_plan(base, n)" in planned and "nonce_plan_ws(base, L.G.bytes" in planned and "L.bytes = L.G.bytes + (nonce ? L.K.bytes : 0);" in planned
    assert "flags must be 0" in capi_secret_shape.function(src, "int ecsimd_sm2_sign_digest(")
    for head in ("int ecsimd_sm2_sm3(", "int ecsimd_sm2_za(", "int ecsimd_sm2_digest("):          # no workspace at all
        body = capi_secret_shape.function(src, head)
        assert "workspace" not in body and "hipMem" not in body and "Synchronize" not in body, head
    verify = capi_secret_shape.function(src, "int sm2_verify_impl(")
    assert "FOR_CHUNKS" not in verify and re.findall(r"launch::(\w+)\(", verify) == ["sm2_digest", "sm2_verify_scalars", "sm2_accept"] and "gc_double_scalar_mult(" in verify
