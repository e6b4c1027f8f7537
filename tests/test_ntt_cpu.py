"""The number-theoretic transform, the part that needs no GPU: tools/ntt_model.py's self-checks (the recursive transform and the pass-by-pass emulation against
the O(n^2) definition, the Fr constants), the fixture byte for byte from the model, the entry points declared in a header of their own and exported beside (not
among) the other sets, a C99 caller, the host-only calls (plan, field_info, bls12_381_fr) against the model with their refusals, and the shipped gfx950
listing of k_ntt: no scratch, no spills."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ntt_model as model   # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_ntt.h")
SYMBOLS = {"ecsimd_ntt_plan", "ecsimd_ntt_field_info", "ecsimd_ntt_bls12_381_fr", "ecsimd_ntt_domain_create", "ecsimd_ntt_domain_destroy", "ecsimd_ntt_forward",
           "ecsimd_ntt_inverse", "ecsimd_ntt_bitrev"}
CAPS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


# ---- the definition
def test_the_models_self_checks():
    assert model.self_check()
    assert model.two_adicity(model.FR) == 32 and model.smallest_non_residue(model.FR) == 5
    assert pow(model.FR_ROOT, 1 << 32, model.FR) == 1 and pow(model.FR_ROOT, 1 << 31, model.FR) == model.FR - 1      # order exactly 2^32
    assert model.default_root(model.FR) == pow(5, (model.FR - 1) >> 32, model.FR) != model.FR_ROOT
    assert model.two_adicity(model.P256_ORDER) == 4 and model.is_prime(model.dense_prime())


def test_the_passes_record_which_buffer_each_wrote():
    x = list(range(1, 33))
    for flags, want in ((0, ["out"]), (3, ["workspace", "out"]), (2, ["workspace", "out", "out"]), (1, ["workspace", "out", "workspace", "out", "out"])):
        trace = []
        assert model.passes(x, model.FR, 5, model.FR_ROOT, flags=flags, trace=trace) == model.forward(x, model.FR, 5, model.FR_ROOT)
        assert [t[0] for t in trace] == want                                  # the input may be `out`: no pass but the last reads and writes one buffer


def test_the_fixture_is_the_models_byte_for_byte():
    assert open(model.VECTORS_PATH).read() == model.vectors_text()
    v = json.load(open(model.VECTORS_PATH))
    assert os.path.getsize(model.VECTORS_PATH) < 64 * 1024
    assert int(v["fr"]["root"], 16) == model.FR_ROOT and v["fr"]["two_adicity"] == 32 and v["fr"]["smallest_non_residue"] == 5
    assert sorted(v["plans"]) == ["0", "2", "3"] and all(len(p) == 24 for p in v["plans"].values())
    for t in v["transforms"]:                                                 # n = 8 and n = 16, on H and on a coset, held to the O(n^2) definition
        x, w = [int(h, 16) for h in t["in"]], model.domain_omega(model.FR, t["log_n"], model.FR_ROOT)
        assert [int(h, 16) for h in t["forward"]] == model.dft(x, w, model.FR, t["shift"])
        assert model.dft([int(h, 16) for h in t["inverse"]], w, model.FR, t["shift"]) == [u % model.FR for u in x]
    assert {(t["log_n"], t["shift"]) for t in v["transforms"]} == {(3, 1), (3, 7), (4, 1), (4, 7)}


# ---- the C ABI
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_ntt_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_ntt")} == declared
    assert {s for s in exported if s.startswith("ecsimd_hip_")} == set(declared_symbols())                # the ecsimd_hip_* set is unchanged: its header's
    assert "ntt" not in open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read().lower()                # ... and nothing was added to that header
    assert '#include "ecsimd_hip.h"' in text and "PUBLIC OR SECRET-INDEPENDENT" in text and "TEST HOOK" in text and "warm-up" in text
    from ecsimd_amd import Engine
    for m in ("ntt_field_info", "ntt_bls12_381_fr", "ntt_plan", "ntt_domain", "ntt_forward", "ntt_inverse", "ntt_bitrev", "ntt_poly_mul"):
        assert callable(getattr(Engine, m)), m
    assert ecsimd_amd.BLS12_381_FR_ROOT == model.FR_ROOT and "BLS12_381_FR_ROOT" in ecsimd_amd.__all__


def test_a_c99_caller_compiles_links_and_plans_without_a_gpu(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_ntt.h"
#include <stddef.h>
#include <stdio.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; ecsimd_ntt_domain* d = NULL; ecsimd_ntt_plan_t p; uint64_t root[4]; int field = -1, s = 0; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_ntt_domain_create(NULL, 2, 4, NULL, NULL, &d);
    rc += ecsimd_ntt_forward(NULL, d, w, w, 1, ECSIMD_NTT_MAX_RADIX_LOG(3)) + ecsimd_ntt_inverse(NULL, d, w, w, 1, 0) + ecsimd_ntt_bitrev(NULL, 4, w, w, 1);
    return rc + ecsimd_ntt_domain_destroy(NULL, d);
  }
  if (ecsimd_ntt_bls12_381_fr(&field, root) != ECSIMD_HIP_OK || ecsimd_ntt_field_info(field, &s, NULL) != ECSIMD_HIP_OK) return 1;
  if (ecsimd_ntt_plan(ECSIMD_NTT_MAX_LOG_N, 1, 0, &p) != ECSIMD_HIP_OK) return 1;
  printf("%d %016llx%016llx%016llx%016llx %d %d %d %d\\n", s, (unsigned long long)root[3], (unsigned long long)root[2], (unsigned long long)root[1], (unsigned long long)root[0],
         p.passes, p.log_radix[0], p.lanes, p.lds_bytes);
  return ecsimd_ntt_plan(ECSIMD_NTT_MAX_LOG_N + 1, 1, 0, &p) == ECSIMD_HIP_ERR_BAD_ARG && ECSIMD_NTT_MAX_PASSES == 24 ? 0 : 2;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = model.plan(24)
    assert r.stdout.split() == ["32", "%064x" % model.FR_ROOT, str(p["passes"]), str(p["log_radix"][0]), str(p["lanes"]), str(p["lds_bytes"])]


# ---- the host-only calls
def test_the_plan_equals_the_models(built):
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    fixture = json.load(open(model.VECTORS_PATH))["plans"]
    for log_n in range(1, 25):
        for flags in CAPS:
            for batch in (1, 3):
                got = Engine.ntt_plan(log_n, batch, flags)
                assert got == model.plan(log_n, batch, flags), (log_n, batch, flags)
                r = got["log_radix"][:got["passes"]]
                assert sum(r) == log_n and max(r) <= (flags or 9) and min(r) >= 1 and got["log_radix"][got["passes"]:] == [0] * (24 - got["passes"])
                assert got["launches"] == got["passes"] and got["workspace_bytes"] == (0 if got["passes"] == 1 else batch * 32 << log_n)
                assert got["lds_bytes"] <= 160 * 1024 // 2 and got["lanes"] == 256
            if str(flags) in fixture:
                rec = fixture[str(flags)][log_n - 1]
                assert rec["log_radix"] == r and rec["passes"] == got["passes"]
    assert Engine.ntt_plan(9)["passes"] == 1 and Engine.ntt_plan(10)["passes"] == 2 and Engine.ntt_plan(18)["passes"] == 2 and Engine.ntt_plan(19)["log_radix"][:3] == [7, 6, 6]
    for log_n, batch, flags in ((0, 1, 0), (25, 1, 0), (-1, 1, 0), (8, 0, 0), (8, 1, 10), (8, 1, 16), (8, 1, -1), (24, (1 << 14) + 1, 0)):
        with pytest.raises(EcsimdHipError):
            Engine.ntt_plan(log_n, batch, flags)
        with pytest.raises(ValueError):
            model.plan(log_n, batch, flags)
    assert built.ecsimd_ntt_plan(8, 1, 0, None) == -1


def test_field_info_and_the_fr_root_equal_the_models(built):
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError, register_modulus
    fid, root = Engine.ntt_bls12_381_fr()
    assert root == model.FR_ROOT and fid == register_modulus(model.FR, prime=True) and Engine.ntt_bls12_381_fr() == (fid, root)
    assert Engine.ntt_field_info(fid) == (32, model.default_root(model.FR))
    assert Engine.ntt_field_info(2) == (model.two_adicity(model.P256_ORDER), model.default_root(model.P256_ORDER))      # P-256's group order
    from helpers import CURVE_PARAMS, P256, SECP256K1
    for field, p in ((3, CURVE_PARAMS[SECP256K1]["n"]), (0, CURVE_PARAMS[P256]["p"]), (1, CURVE_PARAMS[SECP256K1]["p"]), (register_modulus(model.dense_prime(), prime=True), model.dense_prime())):
        assert Engine.ntt_field_info(field) == (model.two_adicity(p), model.default_root(p)), field
    # a modulus not flagged prime is refused, whatever it is; so is an id nobody registered
    for field in (register_modulus(model.FR, prime=False), register_modulus(model.dense_prime() + 2, prime=False), 4000, -1):
        with pytest.raises(EcsimdHipError):
            Engine.ntt_field_info(field)
    assert register_modulus(model.FR, prime=False) != fid


# ---- the shipped ISA
def test_no_kernel_of_the_unit_uses_scratch_or_spills(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_ntt-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_ntt.hip", "ntt.cuh", "gfield.cuh", "field.cuh", "kernels.h"):
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    asm = open(listing).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    assert len(blocks) == 2 and any("k_ntt_pass" in k for k in blocks) and any("k_ntt_bitrev" in k for k in blocks)
    for name, b in blocks.items():
        num = lambda field: int(re.search(r"\.%s:\s+(\d+)" % field, b).group(1))
        assert num("private_segment_fixed_size") == 0 and num("vgpr_spill_count") == 0 and num("sgpr_spill_count") == 0, name
        assert num("vgpr_count") <= 128, name                                # four waves per SIMD fit the registers; LDS allows two workgroups per CU
        assert num("group_segment_fixed_size") == (model.LDS_BYTES if "pass" in name else 0), name
    assert "scratch_" not in asm.split(".amdgpu_metadata")[0].replace("scratch_en", "")
    body = asm.split(".amdgpu_metadata")[0]
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body and "ds_read_b128" in body and "ds_write_b128" in body
    assert not re.search(r"global_(load|store)_dword(x2|x3)?\s", body)           # an element moves as two dwordx4, a table entry too
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_ntt.hip", "ntt.cuh", "ecsimd_ntt.h"):
        assert f in makefile, f
