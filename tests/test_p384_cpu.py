"""NIST P-384, the part that needs no GPU: the entry points are declared in a header of their own, exported beside (not among) the ecsimd_hip_* set, and callable
from C99; the host model the GPU tests take their expected values from (tools/p384_model.py) reproduces RFC 6979 A.2.6 and the fixture bit for bit, agrees
with libcrypto where libcrypto loads, and refuses every one-bit change of a valid signature; the committed table of multiples of G is what the generator
prints; fe384.cuh / p384.cuh, compiled for the HOST, equal Python integers and the model on the extremes (the reduction, both scalar fields, the complete law,
the three window loops); the new kernels exist in the shipped gfx950 listing, the secret ones without scratch memory, and keep their secrets out of every
branch condition, address and lane mask (tools/ct_check.py check_secret_flow), which refuses a branch planted on one bit of d; the host functions wipe the
workspace through the shared step over their own carve."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import p384_model as model      # noqa: E402
import gen_p384_base            # noqa: E402
import capi_secret_shape        # noqa: E402
import ct_check                 # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_p384.h")
SYMBOLS = {"ecsimd_p384_sha384", "ecsimd_p384_pubkey", "ecsimd_p384_ecdh", "ecsimd_p384_ecdsa_verify", "ecsimd_p384_ecdsa_sign", "ecsimd_p384_raw", "ecsimd_p384_raw_inputs",
           "ecsimd_p384_raw_outputs"}
KERNELS = ("13k_p384_sha384", "13k_p384_pubkey", "11k_p384_ecdh", "17k_p384_sign_nonce", "18k_p384_sign_finish", "13k_p384_verify", "10k_p384_raw")
# the pointer arguments whose contents are secret, by position:
#   k_p384_pubkey(d, d_aligned, pub, pub_aligned, ok, n)                              d, the key made of it, the flag made of it
#   k_p384_ecdh(d, d_aligned, peer, peer_aligned, table, z, z_aligned, ok, n)         d, the table (memory is not modelled: what comes back from it counts as secret), z, ok
#   k_p384_sign_nonce(d, d_aligned, digest, digest_aligned, kws, n)                   d, the digest (e and h1 enter K, V and e + r d), k
#   k_p384_sign_finish(d, d_aligned, digest, digest_aligned, kws, sig, sig_aligned, ok, n)
SECRET = {"k_p384_pubkey": [0, 2, 4], "k_p384_ecdh": [0, 4, 5, 7], "k_p384_sign_nonce": [0, 2, 4], "k_p384_sign_finish": [0, 2, 4, 5, 7]}
P, N, G = model.P, model.N, model.G
i2b, b2i = model.i2b, model.b2i
ALL = 2**384 - 1


def fixture():
    return model.load_fixture()


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=3000)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def p_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_p384-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_p384.hip", "p384.cuh", "fe384.cuh", "p384_base.inc", "sha512.cuh"):
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    return open(listing).read()


# ---- the C ABI
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_p384_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_p384")} == declared
    assert {s for s in exported if s.startswith("ecsimd_hip_")} == set(declared_symbols())       # still exactly the declared set
    assert '#include "ecsimd_hip.h"' in text
    assert "p384" not in open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read().lower().replace("-", "")   # nothing was added to the other header
    from ecsimd_amd import Engine
    for m in ("p384_sha384", "p384_pubkey", "p384_ecdh", "p384_ecdsa_verify", "p384_ecdsa_sign", "p384_raw"):
        assert callable(getattr(Engine, m)), m
    ins, outs = (2, 1, 2, 2, 1, 1, 1, 2, 1, 2, 6, 3, 1, 3, 4), (1,) * 9 + (3,) * 6
    assert tuple(built.ecsimd_p384_raw_inputs(op) for op in range(15)) == ins and tuple(built.ecsimd_p384_raw_outputs(op) for op in range(15)) == outs
    for fn in (built.ecsimd_p384_raw_inputs, built.ecsimd_p384_raw_outputs):
        assert fn(-1) == 0 and fn(15) == 0


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "p384_caller.c"), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s


# ---- the model
RFC_X = 0x6B9D3DAD2E1B8C1C05B19875B6659F4DE23C3B667BF297BA9AA47740787137D896D5724E4C70A825F872C9EA60D2EDF5


def test_the_model_reproduces_rfc_6979_a_2_6():
    d = i2b(RFC_X)
    pub, ok = model.pubkey(d)
    assert ok == 1 and pub.hex().upper().startswith("EC3A4E41") and pub[:48].hex().upper().endswith("5480BC13")
    h = model.sha384(b"sample")
    assert model.rfc6979_k(RFC_X, h) == 0x94ED910D1A099DAD3254E9242AE85ABDE4BA15168EAF0CA87A555FD56D10FBCA2907E3E83BA95368623B8C4686915CF9
    sig, ok = model.sign(d, h)
    assert ok == 1 and sig.hex().upper() == ("94EDBB92A5ECB8AAD4736E56C691916B3F88140666CE9FA73D64C4EA95AD133C81A648152E44ACF96E36DD1E80FABE46"
                                             "99EF4AEB15F178CEA1FE40DB2603138F130E740A19624526203B6351D0A3A94FA329C145786E679E7B82C71A38628AC8")
    assert model.verify(pub, h, sig) == 1
    h = model.sha384(b"test")
    sig, ok = model.sign(d, h)
    assert ok == 1 and sig.hex().upper() == ("8203B63D3C853E8D77227FB377BCF7B7B772E97892A80F36AB775D509D7A5FEB0542A7F0812998DA8F1DD3CA3CF023DB"
                                             "DDD0760448D42D8A43AF45AF836FCE4DE8BE06B485E9B61B827C2F13173923E06A739F040649A667BF3B828246BAA5A5")
    assert model.verify(pub, h, sig) == 1


def test_the_curve_constants_and_the_three_laws_agree():
    assert model.mult(N) is model.INF and model.mult_affine(N) is model.INF and model.on_curve(G)
    assert (-pow(P, -1, 2**32)) % 2**32 == 1                                                     # what would make every Montgomery quotient digit the raw word
    assert N.bit_length() == 384 and (2**384 - N).bit_length() == 190
    x = N + 2
    assert x < P and model.lift_x(x) is not None                                                 # the x(R) >= n lane exists
    rng = random.Random(2016)
    pts = [model.INF, G, model.neg(G)] + [model.mult(rng.randrange(1, N)) for _ in range(4)]
    for a in pts:
        assert model.from_proj(model.proj_dbl(model.to_proj(a))) == model.add(a, a)
        for b in pts:
            z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
            pa, pb = tuple(v * z1 % P for v in model.to_proj(a)), tuple(v * z2 % P for v in model.to_proj(b))
            assert model.from_proj(model.proj_add(pa, pb)) == model.add(a, b)
            if b is not model.INF:
                assert model.from_proj(model.proj_add_mixed(pa, b)) == model.add(a, b)
    for k in (0, 1, 2, 15, 16, N - 2, N - 1, N, N + 1, ALL, int("8" * 96, 16), int("7" * 96, 16), int("f" * 96, 16), int("87" * 48, 16), rng.getrandbits(384)):
        assert model.mult(k) == model.mult_affine(k) == model.mult_windowed(k), hex(k)
        digits = model.recode_signed4(k % N)
        assert len(digits) == 97 and all(-8 <= d < 8 for d in digits) and sum(d * 16**i for i, d in enumerate(digits)) == k % N


def test_the_model_agrees_with_libcrypto():
    adj = model.libcrypto()
    if adj is None:
        return                                                                                   # (the comparison exists only where libcrypto loads)
    rng = random.Random(715)
    q = model.mult(rng.randrange(1, N))
    for k in model.EDGE_SCALARS + [N, N + 1, ALL] + [rng.getrandbits(384) for _ in range(20)]:
        assert adj.mult(k) == model.mult(k) and adj.mult(k, q) == model.mult(k, q), hex(k)
    for r in fixture()["verify"]:
        pub, digest, sig = (bytes.fromhex(r[k]) for k in ("pub", "digest", "sig"))
        assert adj.verify(pub, digest, sig) == r["ok"], r["note"]
    assert adj.verify(*model.high_x_case(2)) == 1                                                # x(R) = n + 2: libcrypto accepts r = 2


def test_the_model_reproduces_the_fixture_bit_for_bit():
    fx, stored = fixture(), json.load(open(model.FIXTURE))
    assert len(fx["base"]) + len(fx["ecdh"]) + len(fx["sign"]) + len(fx["verify"]) >= 200 and fx["adjudicated_by_libcrypto"] is True
    again = model.build_fixture(None)
    for key in ("base", "ecdh", "sign", "verify"):
        assert again[key] == stored[key], key
    assert open(model.FIXTURE).read() == model.dump_fixture(stored)
    for r in fx["sign"]:                                                                         # what the stored form leaves out is what it says it is
        assert r["digest"] == model.sha384(bytes.fromhex(r["msg"])).hex() and model.pubkey(bytes.fromhex(r["d"]))[0].hex() == r["pub"]
    assert bytes.fromhex(fx["sign"][0]["d"]) == i2b(RFC_X) and bytes.fromhex(fx["sign"][0]["msg"]) == b"sample" and bytes.fromhex(fx["sign"][1]["msg"]) == b"test"
    assert {r["ok"] for r in fx["verify"]} == {0, 1}


def test_every_one_bit_change_of_a_valid_signature_is_refused():
    d = i2b(RFC_X)
    pub, h = model.pubkey(d)[0], model.sha384(b"sample")
    sig = model.sign(d, h)[0]
    flip = lambda b, bit: bytes(v ^ (1 << (bit % 8)) if q == bit // 8 else v for q, v in enumerate(b))
    assert model.verify(pub, h, sig) == 1
    for bit in range(768):
        assert model.verify(flip(pub, bit), h, sig) == 0, ("pub", bit)
        assert model.verify(pub, h, flip(sig, bit)) == 0, ("sig", bit)
    for bit in range(384):
        assert model.verify(pub, flip(h, bit), sig) == 0, ("digest", bit)


# ---- the table
def test_the_committed_table_is_what_the_generator_prints():
    assert open(os.path.join(CSRC, "p384_base.inc")).read() == gen_p384_base.text()
    rows = gen_p384_base.table()
    assert len(rows) == 25 and all(len(r) == 8 for r in rows) and rows[0][0] == G and rows[24][0] == model.mult(16**96) and rows[5][7] == model.mult(8 * 65536**5)


# ---- the device's arithmetic, compiled for the host
def test_the_field_the_group_law_and_the_window_loops_on_the_host(tmp_path):
    exe = tmp_path / "p384_host_check"
    subprocess.run(["hipcc", "--offload-host-only", "-O0", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "p384_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=1200)
    rng = random.Random(5)
    h = lambda v: "%096x" % v
    reqs, exps = [], []
    pt3 = lambda p: [0, 0, 1] if p is None else [p[0], p[1], 0]

    def ask(op, args, exp):
        reqs.append(op + " " + " ".join(h(a) for a in args)); exps.append(list(exp))
    ops = [0, 1, 2, P - 2, P - 1, P, P + 1, ALL, N - 1, N, N + 1] + [0xffffffff << (32 * j) for j in range(12)] + [ALL ^ (0xffffffff << (32 * j)) for j in range(12)]
    ops += [2**(32 * j) + s for j in range(1, 12) for s in (1, -1)]
    pairs = [(a, b) for a in ops[:14] for b in ops[:14]] + [(a, a) for a in ops] + [(a, rng.getrandbits(384)) for a in ops] + [(rng.getrandbits(384), rng.getrandbits(384)) for _ in range(200)]
    for a, b in pairs:
        ask("mul", [a, b], [a * b % P]); ask("add", [a, b], [(a + b) % P]); ask("sub", [a, b], [(a - b) % P]); ask("scmul", [a, b], [a * b % N])
    for a in ops + [rng.getrandbits(384) for _ in range(50)]:
        ask("sqr", [a], [a * a % P]); ask("neg", [a], [-a % P]); ask("canon", [a], [a % P])
    for a in ops[:11] + [rng.getrandbits(384) for _ in range(5)]:
        ask("inv", [a], [pow(a, P - 2, P)]); ask("scinv", [a], [pow(a, N - 2, N)])
    pts = [None, G, model.neg(G)] + [model.mult(rng.randrange(N)) for _ in range(4)]
    for a in pts:
        ask("pdbl", pt3(a), pt3(model.add(a, a)))
        for b in pts:
            ask("padd", pt3(a) + pt3(b), pt3(model.add(a, b)))
    for x, y, ok in ((G[0], G[1], 1), (G[0], G[1] + 1, 0), (0, 0, 0), (P, G[1], 0), (G[0], P, 0), (ALL, ALL, 0)):
        ask("valid", [x, y], [ok])
    ks = [0, 1, 2, 15, 16, N - 2, N - 1, N, N + 1, ALL, int("8" * 96, 16), int("7" * 96, 16), int("f" * 96, 16), int("87" * 48, 16), 8 << 380, 1 << 383] + [rng.getrandbits(384) for _ in range(10)]
    q = model.mult(rng.randrange(N))
    for k in ks:
        ask("base", [k], pt3(model.mult(k)))
        for pt in (G, model.neg(G), q):
            ask("var", [k, pt[0], pt[1]], pt3(model.mult(k, pt)))
    for u1, u2, pt in [(0, 5, q), (5, 0, q), (0, 0, q), (7, 7, G), (7, N - 7, G), (N - 1, N - 1, q)] + [(rng.randrange(N), rng.randrange(N), q) for _ in range(5)]:
        ask("dmul", [u1, u2, pt[0], pt[1]], pt3(model.add(model.mult(u1), model.mult(u2, pt))))
    out = subprocess.run([str(exe)], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=600)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == len(reqs), out.stderr[-500:]
    wrong = [r[:80] for r, e, l in zip(reqs, exps, lines) if [int(x, 16) for x in l.split()] != e]
    assert not wrong, wrong[:5]


# ---- the shipped ISA
def kernel_blocks(asm):
    meta = asm[asm.index(".amdgpu_metadata"):]
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}


def test_every_new_kernel_is_in_the_listing_and_the_secret_ones_use_no_scratch(p_asm):
    blocks = kernel_blocks(p_asm)
    assert len(blocks) == len(KERNELS), sorted(blocks)
    for k in KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        if k[2:] in SECRET:
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k                  # no scratch memory: what spills stays in the register file
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", hit[0]), k
            assert "scratch_" not in "\n".join(i for b in ct_check.parse_function(p_asm, k[2:]) for i in b[2]), k
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_p384.hip", "fe384.cuh", "p384.cuh", "p384_base.inc", "ecsimd_p384.h"):
        assert f in makefile, f
    import glob                                                                                  # tests/test_isa_guards.py's glob takes the new unit's asm blocks in
    guard = re.search(r'glob\.glob\(os\.path\.join\(ROOT, "build", "csrc", "([^"]+)"\)\)', open(os.path.join(ROOT, "tests", "test_isa_guards.py")).read()).group(1)
    assert any(os.path.basename(f).startswith("k_p384-") for f in glob.glob(os.path.join(ROOT, "build", "csrc", guard)))


@pytest.mark.timeout(1200)
def test_the_secret_kernels_keep_the_secrets_out_of_control_flow_and_addresses(p_asm):
    for k, args in SECRET.items():
        rep = ct_check.check_secret_flow(p_asm, k, secret_args=args)
        assert rep["secret_loads"] >= 3 and not rep["secret_scratch"] and not rep["secret_lds"], (k, rep)
        assert rep["public_branches"] >= 2, (k, rep)                                             # the batch's tail, the alignment flags, the loops


def loop_blocks(asm, kernel):
    """(label, instructions) of the blocks of `kernel` that branch back to themselves."""
    return [(lab, insts) for lab, _, insts in ct_check.parse_function(asm, kernel) if any(i.startswith("s_cbranch_scc") and i.split()[-1] == lab for i in insts)]


def test_the_comb_reads_whole_rows_and_the_window_loop_whole_tables(p_asm):
    dwords = lambda i: int((re.search(r"dwordx(\d+)", i) or [0, 1])[1])
    for kernel in ("k_p384_pubkey", "k_p384_sign_finish"):                                       # the comb: scalar loads of whole entries (24 words), in a loop of their own
        rows = [sum(dwords(i) for i in insts if i.startswith("s_load_dword")) for lab, insts in loop_blocks(p_asm, kernel)]
        rows = [r for r in rows if r]
        assert rows and all(r % 24 == 0 for r in rows), (kernel, rows)
    tables = [sum(1 for i in insts if i.startswith("global_load_dword ")) for lab, insts in loop_blocks(p_asm, "k_p384_ecdh")]
    tables = [t for t in tables if t]
    assert tables and all(t % 36 == 0 for t in tables), tables                                   # whole entries (36 words), in a loop over the entries
    src = open(os.path.join(CSRC, "p384.cuh")).read()
    sel = src[src.index("ECS_HD p384_point p384_table_select("):src.index("// k P for k < n from the lane's table")]
    assert "for (int e = 0; e < 8; ++e)" in sel and "break" not in sel and "table[((size_t)(e * 36 + q)) * lanes + i]" in sel      # the addresses: the entry, the word, the lane -- no window, no digit
    row = src[src.index("ECS_HD p384_affine p384_row_select("):src.index("// acc + (the digit of nibble")]
    assert "for (int e = 0; e < P384_BASE_ENTRIES; ++e)" in row and "break" not in row


def test_the_analysis_refuses_a_branch_planted_on_one_bit_of_d(p_asm):
    """In a COPY of the listing: behind the first load of d in k_p384_pubkey, a compare of the loaded word and a branch on it."""
    start = p_asm.index("k_p384_pubkey")
    m = re.compile(r"\tglobal_load_dwordx4 v\[(\d+):\d+\], v\[\d+:\d+\], off\n").search(p_asm, start)
    label = re.compile(r"^(\.LBB\d+_\d+):", re.M).search(p_asm, m.end()).group(1)
    plant = "\ts_waitcnt vmcnt(0)\n\tv_and_b32_e32 v%s, 4, v%s\n\tv_cmp_ne_u32_e32 vcc, 0, v%s\n\ts_cbranch_vccnz %s\n" % (m.group(1), m.group(1), m.group(1), label)
    planted = p_asm[:m.end()] + plant + p_asm[m.end():]
    with pytest.raises(ct_check.Violation) as exc:
        ct_check.check_secret_flow(planted, "k_p384_pubkey", secret_args=SECRET["k_p384_pubkey"])
    assert "condition" in str(exc.value) or "lane mask" in str(exc.value), exc.value
    ct_check.check_secret_flow(planted, "k_p384_sign_nonce", secret_args=SECRET["k_p384_sign_nonce"])        # a kernel the plant did not touch still passes


# ---- the host layer
def test_the_host_functions_wipe_through_the_shared_step_over_their_own_carve(built):
    src = capi_secret_shape.source()
    for head, plan, launches in (("int ecsimd_p384_ecdsa_sign(", "p384_sign_plan", ["p384_sign_nonce", "p384_sign_finish"]), ("int ecsimd_p384_ecdh(", "p384_table_plan", ["p384_ecdh"])):
        body = capi_secret_shape.function(src, head)
        assert re.findall(r"launch::(\w+)\(", body) == launches, head
        assert "hipMemcpy" not in body and "Synchronize" not in body and "hipMemset" not in body, head        # nothing read back, no wipe of its own
        wipes = re.findall(r"^.*\bwipe_workspace\(.*$", body, re.M)
        assert len(wipes) == 1 and re.fullmatch(r"\s*err = wipe_workspace\(ctx, L\.bytes, hipGetLastError\(\)\);\s*", wipes[0]), (head, wipes)      # no `if` in front
        assert "ensure_workspace(ctx, %s(nullptr, chunk).bytes)" % plan in body and "L = %s(ctx->workspace, chunk);" % plan in body, head
        loop = body[body.index("FOR_CHUNKS("):]
        assert loop.index("launch::" + launches[-1]) < loop.index("wipe_workspace(") and "launch::" not in loop[loop.index("wipe_workspace("):], head
        planned = capi_secret_shape.function(src, plan + "(void* base")
        assert "carve_from(base)" in planned and re.search(r"\bL\.bytes = c\.bytes;", planned), plan
    for head in ("int ecsimd_p384_sha384(", "int ecsimd_p384_pubkey("):                            # no workspace at all
        body = capi_secret_shape.function(src, head)
        assert "workspace" not in body and "hipMem" not in body and "Synchronize" not in body, head
    assert re.search(r"P384_CHUNK = \(size_t\)1 << (\d+);", src).group(1) == "16"
    assert "flags must be 0" in capi_secret_shape.function(src, "int ecsimd_p384_ecdsa_sign(")
