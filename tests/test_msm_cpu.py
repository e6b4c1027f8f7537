"""Multi-scalar multiplication, the part that needs no GPU: the entry points are declared in a header of their own, exported beside (not among) the other
sets, and callable from C99; ecsimd_msm_plan runs on the host alone and equals the schedule of tools/msm_model.py, refusals included; the model's index-level
emulation of the bucket route equals the big-int sum of tests/helpers.py on small adversarial batches, with every virtual lane's count of point operations
under the bound the header documents; the new kernels are in the shipped gfx950 listing with the register and scratch figures DESIGN.md and
profiles/r15/msm_listing.json state."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msm_model as model                                       # noqa: E402
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add, ec_mul   # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_msm.h")
SYMBOLS = {"ecsimd_msm", "ecsimd_msm_point_sum", "ecsimd_msm_plan"}
KERNELS = ("k_msm_digits", "k_msm_slices", "k_msm_combine", "k_msm_chunks", "10k_msm_tree", "k_msm_tree_affineILb1", "k_msm_tree_affineILb0", "k_msm_sanitize", "k_msm_final")   # per curve
COMMON_KERNELS = ("k_msm_zero", "k_msm_scan", "k_msm_scatter")       # no curve in them: k_msm_common.hip, compiled once
PLAN_N = (0, 1, 2, 63, 64, 65, 2**10, 2**16, 2**20, 2**24)
PLAN_BITS = (1, 64, 128, 255, 256)


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


# ---- the C ABI
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_msm(?:_[a-z0-9_]+)?)\s*\(", text))
    assert declared == SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_msm")} == declared
    assert '#include "ecsimd_hip.h"' in text and "PUBLIC DATA ONLY" in text and "NOT for secret scalars" in text
    assert "msm" not in open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read().lower()           # nothing was added to the other headers
    from ecsimd_amd import Engine
    for m in ("msm", "point_sum", "msm_plan"):
        assert callable(getattr(Engine, m)), m


def test_a_c99_caller_compiles_links_and_plans_without_a_gpu(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_msm.h"
#include <stddef.h>
#include <stdio.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* f = NULL; uint32_t* c = NULL; ecsimd_msm_plan_t p; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_msm(NULL, ECSIMD_HIP_SECP256K1, w, w, w, w, w, f, c, 0, 256, ECSIMD_MSM_ALG_AUTO | ECSIMD_MSM_ALG_BUCKETS | ECSIMD_MSM_ALG_LANES);
    return rc + ecsimd_msm_point_sum(NULL, ECSIMD_HIP_P256, w, w, w, w, f, c, 0);
  }
  if (ecsimd_msm_plan(ECSIMD_MSM_MAX_N, 256, ECSIMD_MSM_ALG_AUTO, &p) != ECSIMD_HIP_OK) return 1;
  printf("%d %d %d %u %u %u %u\\n", p.route, p.c, p.windows, (unsigned)p.buckets, (unsigned)p.L, (unsigned)p.m, (unsigned)p.max_chain);
  return ecsimd_msm_plan(ECSIMD_MSM_MAX_N + 1, 256, 0, &p) == ECSIMD_HIP_ERR_BAD_ARG && ECSIMD_MSM_AUTO_THRESHOLD > 0 ? 0 : 2;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert re.search(r"\bU %s\b" % s, out), s
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)                       # ecsimd_msm_plan needs no context and no GPU
    assert r.returncode == 0, r.stderr
    p = model.plan(2**24)
    assert r.stdout.split() == [str(p[f]) for f in ("route", "c", "windows", "buckets", "L", "m", "max_chain")]


# ---- the schedule
def test_the_plan_runs_on_the_host_and_equals_the_models(built):
    from ecsimd_amd import Engine
    from ecsimd_amd.engine import EcsimdHipError
    assert 1 << int(re.search(r"#define ECSIMD_MSM_AUTO_THRESHOLD \(\(size_t\)1 << (\d+)\)", open(HEADER).read()).group(1)) == model.AUTO_THRESHOLD
    assert 1 << int(re.search(r"#define ECSIMD_MSM_MAX_N \(\(size_t\)1 << (\d+)\)", open(HEADER).read()).group(1)) == model.MAX_N == 2**24
    for n in PLAN_N + (3, 4, 5, 9, 33, 257, 4099, 2**22 + 1):
        for bits in PLAN_BITS:
            for flags in (0, 1, 2):
                got, want = Engine.msm_plan(n, bits, flags), model.plan(n, bits, flags)
                assert got == want, (n, bits, flags, got, want)
                assert got["route"] == (flags or (1 if n >= model.AUTO_THRESHOLD else 2))
                if n and got["route"] == 1:
                    assert got["c"] * got["windows"] >= bits > got["c"] * (got["windows"] - 1) and got["buckets"] == 1 << got["c"] and got["buckets"] % got["m"] == 0
                    assert got["L"] & (got["L"] - 1) == 0 and got["L"] * got["L"] <= max(16, 4 * n)      # L <= 2 sqrt(n): the bound is O(sqrt n)
                    assert got["max_chain"] <= 5 * int(n ** 0.5) + 400                                   # ... plus the last lane's constant
    for n, bits, flags in ((1, 0, 0), (1, 257, 0), (1, -1, 1), (2**24 + 1, 256, 0), (2**24 + 1, 256, 2), (8, 256, 3), (8, 256, 4), (8, 256, -1), (8, 256, 1 << 8)):
        with pytest.raises(EcsimdHipError):
            Engine.msm_plan(n, bits, flags)
        with pytest.raises(ValueError):
            model.plan(n, bits, flags)
    assert built.ecsimd_msm_plan(8, 256, 0, None) == -1


# ---- the model's pipeline against the big-int group law
def G(cv):
    return (CURVE_PARAMS[cv]["gx"], CURVE_PARAMS[cv]["gy"])


def neg(cv, P):
    return (P[0], CURVE_PARAMS[cv]["p"] - P[1])


def walk(cv, n, first=1):
    """n distinct points first * G, (first + 1) * G, ... by repeated addition"""
    P = ec_mul(cv, first, G(cv)); out = []
    for _ in range(n):
        out.append(P); P = ec_add(cv, P, G(cv))
    return out


def big_int_sum(cv, ks, pts, bits):
    acc = None
    p = CURVE_PARAMS[cv]["p"]
    for k, (x, y) in zip(ks, pts):
        if (x, y) == (0, 0) or x >= p or y >= p or (y * y - x * x * x - CURVE_PARAMS[cv]["a"] * x - CURVE_PARAMS[cv]["b"]) % p: continue
        acc = ec_add(cv, acc, ec_mul(cv, k % (1 << bits), (x, y)))
    return acc


def adversarial_batches():
    rng = random.Random(0x6d736d)
    out = []
    for cv in (P256, SECP256K1):
        order, p = CURVE_PARAMS[cv]["n"], CURVE_PARAMS[cv]["p"]
        P = ec_mul(cv, rng.getrandbits(200), G(cv))
        k = rng.getrandbits(256)
        L = model.plan(33, 256, 1)["L"]
        assert 8 * L + 1 == 33                                                                        # the all-equal-digits batch of 8 L + 1 terms
        out.append(("all equal, 8 L + 1", cv, [k] * 33, [P] * 33, 256, 0))
        for n in (L - 1, L, L + 1, 2 * L + 1):
            out.append((f"all equal, n = {n}", cv, [k] * n, [P] * n, 64, 0))
        n = 300; L2 = model.plan(n, 16, 1)["L"]
        out.append((f"all equal, n = {n}, L = {L2}", cv, [0x1357] * n, [P] * n, 16, 0))
        pts = walk(cv, 6)
        ks = [rng.getrandbits(256) for _ in pts]
        out.append(("k P and k (-P)", cv, ks + ks, pts + [neg(cv, Q) for Q in pts], 256, 0))
        ks = [rng.randrange(1, order) for _ in pts]
        out.append(("k P and (n - k) P", cv, ks + [order - v for v in ks], pts + pts, 256, 0))
        out.append(("all k = 0", cv, [0] * 7, walk(cv, 7), 256, 0))
        out.append(("all points at infinity", cv, [rng.getrandbits(256) for _ in range(7)], [(0, 0)] * 7, 256, 0))
        for bits in (256, 128, 13, 1):
            out.append((f"k = 2^{bits} - 1", cv, [(1 << 256) - 1] * 5, walk(cv, 5), bits, 0))
        c = model.plan(9, 255, 1)["c"]
        out.append(("one window: the lowest, the highest, a partial top one", cv, [(1 << c) - 1, ((1 << c) - 1) << (c * (model.plan(9, 255, 1)["windows"] - 1)), 1 << 254] * 3, walk(cv, 9), 255, 0))
        out.append(("garbage above bits", cv, [rng.getrandbits(256) | (1 << 255) for _ in range(9)], walk(cv, 9), 128, 0))
        pl = model.plan(4099, 16, 1)
        m, top = pl["m"], pl["buckets"] - 1
        assert pl["buckets"] > m + 1 and pl["c"] == 8
        edge = [m - 1, m, m + 1, top]
        out.append(("chunk edges of the reduction", cv, [edge[i % 4] | (edge[(i + 1) % 4] << 8) for i in range(4099)], walk(cv, 4099), 16, 0))
        bad = [(P[0], (P[1] + 1) % p), (p, P[1]), (P[0], p), (P[0], p + 5), (0, 1)]
        pts = walk(cv, 8); pts[1:6] = bad
        out.append(("invalid points", cv, [rng.getrandbits(256) for _ in pts], pts, 256, 5))
        for n in (1, 2, 63, 64, 65):
            out.append((f"random, n = {n}", cv, [rng.getrandbits(64) for _ in range(n)], walk(cv, n, 3), 64, 0))
    return out


def test_the_models_pipeline_equals_the_big_int_sum_and_keeps_the_serial_bound():
    rng = random.Random(5)
    for name, cv, ks, pts, bits, invalid in adversarial_batches():
        want = big_int_sum(cv, ks, pts, bits)
        shuffled = lambda idx: rng.sample(idx, len(idx))                                              # the order inside a bucket is free
        for order in (None, shuffled):
            got, bad, stats = model.msm_buckets(cv, ks, pts, bits, order)
            assert got == want and bad == invalid, (name, cv)
            S = model.schedule(len(ks), bits, 1)
            n = len(ks)
            assert stats.get("slices", 0) <= S["L"], (name, stats)
            assert stats.get("combine", 0) <= -(-n // S["L"]) + 1, (name, stats)
            assert stats.get("chunks", 0) <= 2 * S["m"] + 2 * S["c"] and stats.get("tree", 0) <= model.TREE_FAN - 1 and stats["final"] == S["windows"] * (S["c"] + 1), (name, stats)
            assert max(stats.values()) <= S["max_chain"], (name, stats, S["max_chain"])
        if name.startswith("all equal, n = 300"):
            assert stats["slices"] == S["L"] == 8 and 38 == -(-300 // 8) <= stats["combine"] <= 39        # the bound is reached, not merely kept: one bucket holds all n
        if name.startswith("all equal, 8 L + 1"):
            assert stats["slices"] == 4 and stats["combine"] >= 9
        assert model.msm_reference(cv, ks, pts, bits) == want
        if bits == 256 and len(ks) <= 16:
            got, bad, st = model.point_sum(cv, pts)
            acc = None
            for Q in pts:
                if model.classify(cv, Q) == 1: acc = ec_add(cv, acc, Q)
            assert got == acc and bad == invalid and st.get("front", 0) <= model.TREE_FAN


# ---- the shipped ISA
def kernel_blocks(asm):
    meta = asm[asm.index(".amdgpu_metadata"):]
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}


def unit_figures(unit, sources, kernels):
    listing = os.path.join(ROOT, "build", "csrc", f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in sources:
        assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, f)), f
    blocks = kernel_blocks(open(listing).read())
    out = {}
    for k in kernels:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        num = lambda field: int(re.search(r"\.%s:\s+(\d+)" % field, hit[0]).group(1))
        short = re.sub(r"^\d+", "", k).replace("ILb1", "<validate>").replace("ILb0", "<plain>")
        out[short] = dict(vgprs=num("vgpr_count"), sgprs=num("sgpr_count"), scratch_bytes=num("private_segment_fixed_size"),
                          spilled_vgprs=num("vgpr_spill_count"), lds_bytes=num("group_segment_fixed_size"))
    return out, len(blocks)


def listing_figures():
    out = {}
    common, blocks = unit_figures("k_msm_common", ("k_msm_common.hip", "msm_stages.cuh", "field.cuh", "kernels.h"), COMMON_KERNELS)
    assert blocks == len(COMMON_KERNELS) + 1                                                           # ... and the AND of verdict bytes, which is no stage of the sum
    for curve in ("p256", "secp256k1"):
        own, blocks = unit_figures(f"k_msm_{curve}", (f"k_msm_{curve}.hip", "k_msm.inc", "msm_stages.cuh", "point.cuh", "field.cuh", "kernels.h"), KERNELS)
        assert blocks == len(KERNELS) == 9
        for name, f in {**own, **common}.items():                                                      # the common kernels serve both curves: the record has them under each
            out.setdefault(name, {})[curve] = f
    return out


def test_the_new_kernels_are_in_the_listing_with_the_figures_the_documents_state(built):
    got = listing_figures()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "r15", "msm_listing.json")))["kernels"]
    assert got == recorded
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, per_curve in got.items():
        for curve, f in per_curve.items():
            assert f["spilled_vgprs"] == 0 and f["scratch_bytes"] <= 112, (name, curve, f)               # no more stack than the other public-data kernels
            assert f["vgprs"] <= 256, (name, curve, f)                                                 # two waves per SIMD at the least
        row = "| `%s` | %d / %d | %d / %d |" % (name, per_curve["p256"]["vgprs"], per_curve["secp256k1"]["vgprs"], per_curve["p256"]["scratch_bytes"],
                                                per_curve["secp256k1"]["scratch_bytes"])
        assert row in design, row
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("k_msm_p256.hip", "k_msm_secp256k1.hip", "k_msm_common.hip", "k_msm.inc", "msm_stages.cuh", "ecsimd_msm.h"):
        assert f in makefile, f
