"""X25519, the part that needs no GPU: the entry points are declared in a header of their own, exported beside (not among) the other sets, and callable from
C99; the host model the GPU tests take their expected values from (tools/x25519_model.py) gives the fixture and RFC 7748's values bit for bit and agrees
with libcrypto where libcrypto loads, failures included; the Edwards route equals the ladder on 9 and the two conversions commute with the public keys; the
device's word arithmetic, emulated, equals the integers on the extremes; the new kernels exist in the shipped gfx950 listing, the secret ones without scratch
memory or LDS, and keep their secrets out of every branch condition, address and lane mask (tools/ct_check.py check_secret_flow), which refuses a planted
branch on one bit of the scalar; the host functions touch neither the workspace nor the host."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as ed      # noqa: E402
import x25519_model as model    # noqa: E402
import capi_secret_shape        # noqa: E402
import ct_check                 # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_x25519.h")
SYMBOLS = {"ecsimd_x25519", "ecsimd_x25519_base", "ecsimd_x25519_from_ed25519_pk", "ecsimd_x25519_from_ed25519_seed", "ecsimd_x25519_raw", "ecsimd_x25519_raw_inputs",
           "ecsimd_x25519_raw_outputs"}
KERNELS = ("8k_x25519E", "13k_x25519_base", "19k_x25519_from_ed_pk", "21k_x25519_from_ed_seed", "12k_x25519_raw")
SECRET_KERNELS = (KERNELS[0], KERNELS[1], KERNELS[3])
# k_x25519(scalar, scalar_aligned, u, u_aligned, out, out_aligned, ok, n): the scalar, the output and the flag made of it; u is argument 2
LADDER, LADDER_SECRETS, LADDER_U = "8k_x25519E", [0, 4, 6], 2
# k_x25519_base(gmod BY VALUE, scalar, scalar_aligned, out, out_aligned, n)
COMB, COMB_SECRETS = "k_x25519_base", [1, 3]
# k_x25519_from_ed_seed(seed, seed_aligned, scalar, scalar_aligned, n)
SEED, SEED_SECRETS = "k_x25519_from_ed_seed", [0, 2]
P, L = model.P, model.L
le32 = model.le32
LADDER_SCALARS = (0, 1, 2, 3, 7, 8, L - 1, L, L + 1, 2 * L, 2**252, 2**254, 2**255 - 1)


def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "x25519_vectors.json")))


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def x_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_x25519-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_x25519.hip", "x25519.cuh", "ed25519.cuh", "fe25519.cuh", "ed25519_base.inc", "sha512.cuh"):
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    return open(listing).read()


# ---- the C ABI
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_x25519(?:_[a-z0-9_]+)?)\s*\(", text))
    assert declared == SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_x25519")} == declared
    assert '#include "ecsimd_hip.h"' in text
    assert "25519" not in open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()                 # nothing was added to the other headers
    assert "x25519" not in open(os.path.join(ROOT, "include", "ecsimd_ed25519.h")).read().lower()
    from ecsimd_amd import Engine
    for m in ("x25519", "x25519_base", "x25519_from_ed25519_pk", "x25519_from_ed25519_seed", "x25519_raw"):
        assert callable(getattr(Engine, m)), m
    for name, fn, want in (("inputs", built.ecsimd_x25519_raw_inputs, (1, 2, 1)), ("outputs", built.ecsimd_x25519_raw_outputs, (1, 1, 2))):
        assert tuple(fn(op) for op in range(3)) == want and fn(-1) == 0 and fn(3) == 0, name


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_x25519.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint8_t* b = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_x25519(NULL, b, b, b, NULL, 0);
    rc |= ecsimd_x25519_base(NULL, b, b, 0);
    rc |= ecsimd_x25519_from_ed25519_pk(NULL, b, b, b, 0);
    rc |= ecsimd_x25519_from_ed25519_seed(NULL, b, b, 0);
    rc |= ecsimd_x25519_raw(NULL, ECSIMD_X25519_RAW_LADDER, b, b, 0);
    return rc + ecsimd_x25519_raw_inputs(ECSIMD_X25519_RAW_FE_MUL_SMALL) + ecsimd_x25519_raw_outputs(ECSIMD_X25519_RAW_ED_TO_MONT);
  }
  return 0;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s


# ---- the host model and the fixture
def test_the_model_gives_the_fixture_and_rfc_7748_bit_for_bit():
    fx = fixture()
    cases = fx["cases"]
    assert len(cases) >= 80 and sum(c["source"].startswith("RFC 7748") for c in cases) == 6
    assert sum("twist" in c["source"] for c in cases) >= 12 and sum(c["ok"] == 0 for c in cases) >= 14
    for c in cases:
        out = model.x25519(bytes.fromhex(c["scalar"]), bytes.fromhex(c["u"]))
        assert out.hex() == c["out"] and model.ok_of(out) == c["ok"], c
    v1, v2 = model.RFC7748_VECTORS
    assert (cases[0]["scalar"], cases[0]["u"], cases[0]["out"]) == v1 and (cases[1]["scalar"], cases[1]["u"], cases[1]["out"]) == v2
    assert v1[2] == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552" and v2[2] == "95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957"
    assert fx["iterated"] == {"1": "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079", "1000": "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"}
    assert {str(i): v.hex() for i, v in model.iterate(1000).items()} == fx["iterated"]
    d = fx["dh"]
    assert d == model.RFC7748_DH and d["shared"] == "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"
    a, b = bytes.fromhex(d["a"]), bytes.fromhex(d["b"])
    assert model.x25519_base(a).hex() == d["a_public"] == model.x25519(a, model.NINE).hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    assert model.x25519_base(b).hex() == d["b_public"] == model.x25519(b, model.NINE).hex() == "de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f"
    assert model.x25519(a, bytes.fromhex(d["b_public"])).hex() == model.x25519(b, bytes.fromhex(d["a_public"])).hex() == d["shared"]


def both_top_bits(u):
    return (le32(u), le32(u | (1 << 255)))


def test_the_model_agrees_with_libcrypto():
    ossl = model.libcrypto()
    if ossl is None:
        return                                                                                        # (the comparison exists only where libcrypto loads)
    rng = random.Random(7748)
    for _ in range(200):
        k, u = rng.randbytes(32), rng.randbytes(32)
        assert model.x25519(k, u) == ossl.derive(k, u)
        assert model.x25519_base(k) == ossl.public(k) == model.x25519(k, model.NINE)
    failed = 0
    for u in model.SMALL_ORDER_U:                                                                     # libcrypto fails exactly where the model gives zero
        for enc in both_top_bits(u):
            k = rng.randbytes(32)
            assert model.x25519(k, enc) == bytes(32) and ossl.derive(k, enc) is None, enc.hex()
            failed += 1
    assert failed == 14
    for u in [P - 3 + i for i in range(22)] + [2**255 - 1]:                                           # non-canonical u: the residue counts
        for enc in both_top_bits(u):
            k = rng.randbytes(32)
            got = ossl.derive(k, enc)
            assert (got or bytes(32)) == model.x25519(k, enc) == model.x25519(k, le32(u % P)), enc.hex()
            assert (got is None) == (u % (1 << 255) in model.SMALL_ORDER_U)


# ---- the other route and the conversions
def test_the_edwards_route_is_the_ladder_on_nine_and_the_conversions_commute():
    rng = random.Random(9)
    for k in LADDER_SCALARS:                                                                          # unclamped: the identity maps to 0
        assert model.ladder(k, 9) == model.edwards_base(k), k
    assert model.ladder(L, 9) == 0 == model.ladder(0, 9) and model.ladder(1, 9) == 9 == model.ladder(L + 1, 9) == model.ladder(L - 1, 9)
    for k in [bytes(32), bytes([0xff]) * 32] + [rng.randbytes(32) for _ in range(20)]:
        assert model.x25519_base(k) == model.x25519(k, model.NINE)
        assert model.clamp(int.from_bytes(k, "little")) % L != 0
    for _ in range(12):
        seed = rng.randbytes(32)
        pk = ed.pubkey(seed)
        u, ok = model.from_ed25519_pk(pk)
        assert ok == 1 and model.x25519_base(model.from_ed25519_seed(seed)) == u
        assert model.from_ed25519_pk(ed.encode(ed.pt_neg(ed.decode(pk)))) == (u, 1)                 # the map drops the sign of x
        y = int.from_bytes(pk, "little") & (2**255 - 1)
        assert int.from_bytes(u, "little") == (1 + y) * pow(1 - y, P - 2, P) % P
    assert int.from_bytes(model.from_ed25519_seed(bytes(32)), "little") == ed.expand(bytes(32))[0]
    for e in ed.SMALL_ORDER + (le32(P + 1), le32(2), le32(1 | (1 << 255))):
        assert model.from_ed25519_pk(e) == (bytes(32), 0), e.hex()
    assert model.from_ed25519_pk(ed.encode(ed.B)) == (model.NINE, 1)


def test_the_small_order_words_in_the_device_source_are_the_models():
    src = open(os.path.join(CSRC, "x25519.cuh")).read()
    table = re.search(r"S\[3\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [b"".join(int(x, 16).to_bytes(4, "little") for x in re.findall(r"0x([0-9a-fA-F]{8})u", row)) for row in re.findall(r"\{([^{}]*)\}", table)]
    assert rows == [ed.SMALL_ORDER[1], ed.SMALL_ORDER[4], ed.SMALL_ORDER[6]]
    assert "X25519_A24 = 121665u" in src and (486662 - 2) // 4 == model.A24


# ---- the device's arithmetic on eight 32-bit words
EXTREMES = (2**256 - 1, 2**256 - 38, 2**256 - 39, P, P + 1, P - 1, 0, 1, 2**255, 2**255 - 1)


def test_word_level_emulation_of_mul_small_and_one_ladder_step():
    rng = random.Random(121665)
    for a in EXTREMES + tuple(rng.getrandbits(256) for _ in range(200)):
        got = model.int_of(model.w_mul_small(model.words_of(a), model.A24))
        assert got < 2**256 and got % P == a * model.A24 % P, hex(a)
    assert 121665 * (2**32 - 1) >> 32 < 2**17                                                         # the top word of the product
    pool = EXTREMES + tuple(rng.getrandbits(256) for _ in range(6))
    for _ in range(400):
        x1, x2, z2, x3, z3 = (rng.choice(pool) for _ in range(5))
        nx2, nz2, nx3, nz3 = (model.int_of(w) for w in model.w_ladder_step(*(model.words_of(v) for v in (x1, x2, z2, x3, z3))))
        a, b = x2 + z2, x2 - z2
        e = a * a - b * b
        c, d = x3 + z3, x3 - z3
        assert nx2 % P == (a * a * b * b) % P and nz2 % P == e * (a * a + model.A24 * e) % P
        assert nx3 % P == (d * a + c * b) ** 2 % P and nz3 % P == x1 * (d * a - c * b) ** 2 % P
    for v in EXTREMES:                                                                                # all five operands the same extreme
        model.w_ladder_step(*(model.words_of(v),) * 5)


# ---- the shipped ISA
def kernel_blocks(asm):
    meta = asm[asm.index(".amdgpu_metadata"):]
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}


def test_every_new_kernel_is_in_the_listing_and_the_secret_ones_use_no_scratch(x_asm):
    blocks = kernel_blocks(x_asm)
    assert len(blocks) == len(KERNELS), sorted(blocks)
    for k in KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        if k in SECRET_KERNELS:
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k
            assert re.search(r"\.vgpr_spill_count:\s+0\b", hit[0]), k
            assert re.search(r"\.group_segment_fixed_size:\s+0\b", hit[0]), k
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_x25519.hip", "x25519.cuh", "ecsimd_x25519.h"):
        assert f in makefile, f


def test_the_secret_kernels_keep_the_secrets_out_of_control_flow_and_addresses(x_asm):
    rep = ct_check.check_secret_flow(x_asm, LADDER, secret_args=LADDER_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]          # the scalar: 32 bytes
    assert rep["public_branches"] >= 2                                                               # the batch's tail, the alignment flags, the loop
    rep = ct_check.check_secret_flow(x_asm, LADDER, secret_args=LADDER_SECRETS + [LADDER_U])        # ... and with the peer's u secret as well
    assert rep["secret_loads"] >= 4 and not rep["secret_scratch"] and not rep["secret_lds"]
    rep = ct_check.check_secret_flow(x_asm, COMB, secret_args=COMB_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]
    rep = ct_check.check_secret_flow(x_asm, SEED, secret_args=SEED_SECRETS)
    assert rep["secret_loads"] >= 2 and not rep["secret_scratch"] and not rep["secret_lds"]


PLANT_ANCHOR = "  ed_store32(out + 32 * i, r, out_aligned);\n"
PLANT = "  if (k.w[3] & 4u) out[32 * i + 1] = 1;\n"


def test_the_analysis_refuses_a_planted_branch_on_one_bit_of_the_scalar(tmp_path):
    src = open(os.path.join(CSRC, "k_x25519.hip")).read()
    assert src.count(PLANT_ANCHOR) == 1
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC]
    unit, out = tmp_path / "planted.hip", tmp_path / "planted.s"
    unit.write_text(src.replace(PLANT_ANCHOR, PLANT_ANCHOR + PLANT))
    subprocess.run(["hipcc"] + flags + [str(unit), "-o", str(out)], check=True, capture_output=True, timeout=1200)
    asm = out.read_text()
    with pytest.raises(ct_check.Violation) as exc:
        ct_check.check_secret_flow(asm, LADDER, secret_args=LADDER_SECRETS)
    assert "lane mask" in str(exc.value) or "condition" in str(exc.value), exc.value
    ct_check.check_secret_flow(asm, COMB, secret_args=COMB_SECRETS)                                   # the kernels the mutation did not touch still pass
    ct_check.check_secret_flow(asm, SEED, secret_args=SEED_SECRETS)


# ---- the host layer
def test_the_host_functions_use_no_workspace_and_never_touch_the_host(built):
    src = capi_secret_shape.source()
    for head in ("int ecsimd_x25519(", "int ecsimd_x25519_base(", "int ecsimd_x25519_from_ed25519_pk(", "int ecsimd_x25519_from_ed25519_seed(", "int ecsimd_x25519_raw("):
        body = capi_secret_shape.function(src, head)
        for word in ("ensure_workspace", "hipMemcpy", "hipMemset", "Synchronize", "workspace", "NO_COMPAT", "refuse_compat"):
            assert word not in body, (head, word)
        assert "FOR_CHUNKS(first, m, n, X25519_CHUNK)" in body and "bad(ctx" in body, head
    assert "launch::x25519_base(ctx->stream, *ed25519_order()" in capi_secret_shape.function(src, "int ecsimd_x25519_base(")
    assert re.search(r"X25519_CHUNK = \(size_t\)1 << (\d+);", src).group(1) == "20"
