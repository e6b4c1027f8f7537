"""Ed25519 batch verification without a GPU (include/ecsimd_ed25519_batch.h): the host model of the cofactored rule and of the batch method against its own
per-lane verdicts over tests/golden/ed25519_verdicts.json, the tag midstates the device source holds as literals, the two host-only plans, the C boundary."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ed25519_model as ed             # noqa: E402
import ed25519_batch_model as model    # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_ed25519_batch.h")
NAMES = ("ecsimd_ed25519_msm", "ecsimd_ed25519_msm_plan", "ecsimd_ed25519_verify_cofactored", "ecsimd_ed25519_batch_plan", "ecsimd_ed25519_verify_batch",
         "ecsimd_ed25519_batch_randomizers")
SMALL, AUTO, MSM, LANES = 1, 0, 2, 4
MAX_N = (1 << 24) - 1
BAD_ARG = -1
PLAN_SIZES = (0, 1, 2, 16, 17, 257, 1 << 20, MAX_N)


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def records():
    recs = json.load(open(os.path.join(ROOT, "tests", "golden", "ed25519_verdicts.json")))["records"]
    out = []
    for r in recs:
        pk, msg, sig = bytes.fromhex(r["public_key"]), bytes.fromhex(r["message"]), bytes.fromhex(r["signature"])
        out.append(dict(kind=r["kind"], pk=pk, msg=msg, sig=sig, model=r["model"], strict=r["model_strict"],
                        cof=int(model.verify_cofactored(pk, msg, sig)), cof_strict=int(model.verify_cofactored(pk, msg, sig, True))))
    return out


def cols(lanes):
    return [x["pk"] for x in lanes], [x["msg"] for x in lanes], [x["sig"] for x in lanes]


# ---- the rule
def test_cofactorless_accepted_implies_cofactored_accepted_over_the_whole_fixture(records):
    assert len(records) == 1019
    assert [r for r in records if r["model"] and not r["cof"]] == []
    assert [r for r in records if r["strict"] and not r["cof_strict"]] == []
    assert all(r["cof_strict"] <= r["cof"] for r in records)


def test_the_676_cofactored_only_records_are_accepted(records):
    only = [r for r in records if r["cof"] and not r["model"]]
    kinds = {}
    for r in only:
        kinds[r["kind"]] = kinds.get(r["kind"], 0) + 1
    assert len(only) == 676 and kinds.pop("small order") == 452 and sum(kinds.values()) == 224 and set(kinds) == set(ed.MIXED_KINDS), kinds
    # with the flag every small-order record is refused, and the mixed-order ones (no small-order encoding among them) are not
    assert not any(r["cof_strict"] for r in records if r["kind"] == "small order")
    assert all(r["cof_strict"] for r in only if r["kind"] in ed.MIXED_KINDS)


def test_strict_decoding_is_not_zip215(records):
    """A non-canonical A or R is refused whatever the equation says."""
    for r in records:
        if r["kind"] in ("A non-canonical", "R non-canonical", "A refused", "s = L", "s + k L"):
            assert not r["cof"], r["kind"]
    ident = ed.SMALL_ORDER[0]
    assert model.verify_cofactored(ident, b"m", ident + bytes(32))
    assert not model.verify_cofactored(ident, b"m", (ed.P + 1).to_bytes(32, "little") + bytes(32))        # the same point, y + p
    assert not model.verify_cofactored((ed.P + 1).to_bytes(32, "little"), b"m", ident + bytes(32))
    assert not model.verify_cofactored(ident, b"m", (2).to_bytes(32, "little") + bytes(32))               # y = 2 is on no point


# ---- the batch
def test_the_batch_verdict_is_the_and_of_the_per_lane_verdicts(records):
    assert model.batch_verify([], [], []) and model.batch_verify_lanes([], [], [])
    good = [r for r in records if r["cof"]]
    bad = [r for r in records if not r["cof"]]
    by_kind = {}
    for r in bad:
        by_kind.setdefault(r["kind"], r)
    assert len(by_kind) >= 10
    # accepted batches of several compositions: honest only, cofactored-only only, both
    honest = [r for r in good if r["kind"] == "valid"]
    mixed = [r for r in good if r["kind"] in ed.MIXED_KINDS and not r["model"]]
    small = [r for r in good if r["kind"] == "small order" and not r["model"]]
    for lanes in (honest[:1], honest[:6], mixed[:7], small[:5], honest[:3] + mixed[:3] + small[:3], mixed[3:20]):
        assert model.batch_verify_lanes(*cols(lanes)) and model.batch_verify(*cols(lanes)), [x["kind"] for x in lanes]
    # one refused lane of every kind, at either end
    base = honest[:2] + mixed[:2]
    for kind, r in by_kind.items():
        for lanes in ([r] + base, base + [r]):
            assert not model.batch_verify_lanes(*cols(lanes)) and not model.batch_verify(*cols(lanes)), kind
    # the flag
    assert model.batch_verify(*cols(small[:3]), reject_small_order=False) and not model.batch_verify(*cols(small[:3]), reject_small_order=True)
    assert model.batch_verify(*cols(mixed[:4]), reject_small_order=True) == model.batch_verify_lanes(*cols(mixed[:4]), reject_small_order=True) == True  # noqa: E712


def test_the_verdict_does_not_depend_on_the_lane_order(records):
    every = [r for r in records if r["kind"] in ed.MIXED_KINDS and r["cof"] and not r["model"]]
    mixed = every[:9]
    z = model.randomizers(*cols(mixed))
    turned = mixed[4:] + mixed[:4]
    assert z != model.randomizers(*cols(turned))
    assert model.batch_verify(*cols(mixed)) and model.batch_verify(*cols(turned))
    # the cofactorless sum of the same lanes is NOT a function of the batch: without the 8 some weights accept and some refuse
    # each lane's defect R + [h]A - [s]B is a torsion point, and odd weights can make two of them cancel or not
    def defect(x):
        h = int.from_bytes(model.digest(x["pk"], x["msg"], x["sig"]), "little") % ed.L
        return ed.pt_add(ed.pt_add(ed.decode(x["sig"][:32]), ed.pt_mul(h, ed.decode(x["pk"]))), ed.pt_neg(ed.base_point_mul(int.from_bytes(x["sig"][32:], "little"))))
    defects = [defect(x) for x in every[::12]]                            # (a sample across the classes of the fixture: orders 2, 4 and 8)
    assert {ed.order_of(d) for d in defects} == {2, 4, 8}
    both = [(i, j) for i in range(len(defects)) for j in range(i + 1, len(defects))
            if {ed.pt_eq(ed.pt_add(defects[i], ed.pt_mul(w, defects[j])), ed.IDENTITY) for w in (1, 3, 5, 7)} == {True, False}]
    assert both, "no pair of these lanes whose cofactorless sum depends on the weights"


def test_errors_that_cancel_under_unit_weights_are_refused_by_the_randomizers(records):
    honest = [r for r in records if r["kind"] == "valid"][:6]
    lanes = [dict(x) for x in honest]
    for i, d in ((1, 1), (4, -1)):
        s = (int.from_bytes(lanes[i]["sig"][32:], "little") + d) % ed.L
        lanes[i]["sig"] = lanes[i]["sig"][:32] + s.to_bytes(32, "little")
    assert not model.batch_verify_lanes(*cols(lanes))
    # with z_i = 1 the products z_i h_i and the sum of the s are what they were: the unweighted equation holds
    assert model.batch_verify(*cols(lanes), z=[1] * 6) and not model.batch_verify(*cols(lanes))


def test_randomizers_are_odd_below_2_128_and_bind_every_lane(records):
    lanes = [r for r in records if r["kind"] in ("valid", "flip s", "A refused", "small order")][:40]
    z = model.randomizers(*cols(lanes))
    assert len(z) == 40 and all(x & 1 and x < 1 << 128 for x in z) and len(set(z)) == 40
    other = [dict(x) for x in lanes]
    other[17]["msg"] = other[17]["msg"] + b"\x00"
    assert all(a != b for a, b in zip(z, model.randomizers(*cols(other))))
    assert all(a != b for a, b in zip(z, model.randomizers(*cols(lanes[:39]))))
    assert model.randomizers([], [], []) == []
    # the tree: 17 leaves are two levels, and the root of one leaf is the leaf
    leaves = [bytes([i]) * 32 for i in range(17)]
    level1 = [model.tagged_hash(model.TAG_NODE, b"".join(leaves[:16])), model.tagged_hash(model.TAG_NODE, leaves[16])]
    assert model.root(leaves) == model.tagged_hash(model.TAG_NODE, level1[0] + level1[1]) and model.root(leaves[:1]) == leaves[0]


def test_the_models_sum_is_the_integer_combination():
    tors = ed.torsion()
    pts = [ed.encode(ed.mixed(ed.base_point_mul(5 + i), t)) for i, (_, t, _) in enumerate(tors)]
    ks = [ed.L + 3 + i for i in range(8)]
    enc, finite, invalid = model.msm_encoded(ks, pts)
    acc = ed.IDENTITY
    for i, (_, t, _) in enumerate(tors):
        acc = ed.pt_add(acc, ed.pt_add(ed.base_point_mul((5 + i) * ks[i]), ed.pt_mul(ks[i] % 8, t)))
    assert enc == ed.encode(acc) and finite == 1 and invalid == 0
    assert model.msm_encoded([ed.L], [ed.encode(ed.B)]) == (ed.SMALL_ORDER[0], 0, 0)
    assert model.msm_encoded([7, 9], [(2).to_bytes(32, "little"), ed.encode(ed.B)]) == (ed.encode(ed.base_point_mul(9)), 1, 1)
    assert model.msm_encoded([0xff], [ed.encode(ed.B)], bits=4) == (ed.encode(ed.base_point_mul(15)), 1, 0)


# ---- the device source
def test_the_midstates_in_the_device_source_are_hashlibs():
    src = open(os.path.join(CSRC, "k_msm_ed25519.hip")).read()
    table = re.search(r"ED25519_BATCH_MID\[4\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [[int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", row)] for row in re.findall(r"\{([^{}]*)\}", table)]
    assert len(rows) == 4 and all(len(r) == 8 for r in rows)
    assert model.DEVICE_TAGS == (model.TAG_LEAF, model.TAG_NODE, model.TAG_SEED, model.TAG_A)
    assert 'tag = "ecsimd/ed25519-batch/leaf", ".../node", ".../seed", ".../a"' in src
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bip340_model as b340
    for tag, row in zip(model.DEVICE_TAGS, rows):
        assert tag.startswith("ecsimd/ed25519-batch/")
        assert row == model.midstate(tag) == list(b340.midstate(tag)), tag
        for length in (0, 40, 64, 96, 512):
            data = bytes(range(256)) * 2
            assert b340.finish_from_midstate(row, data[:length]) == model.tagged_hash(tag, data[:length])
    t = hashlib.sha256(b"ecsimd/ed25519-batch/a").digest()
    assert model.tagged_hash(model.TAG_A, b"xyz") == hashlib.sha256(t + t + b"xyz").digest()


# ---- the plans
def plan(lib, n, msg_bytes=32, flags=AUTO):
    from ecsimd_amd.engine import Ed25519BatchPlan
    p = Ed25519BatchPlan()
    rc = lib.ecsimd_ed25519_batch_plan(C.c_size_t(n), C.c_size_t(msg_bytes), C.c_int(flags), C.byref(p))
    return rc, p


def threshold():
    m = re.search(r"#define ECSIMD_ED25519_BATCH_AUTO_THRESHOLD\s+(.*)", open(HEADER).read()).group(1).strip()
    return 1 << int(re.fullmatch(r"\(\(size_t\)1 << (\d+)\)", m).group(1))


def tree_passes(c):
    p = 0
    while c > 1:
        c = (c + 15) // 16; p += 1
    return p


def msm_launches(n, bits):
    """The header's M(n, bits), restated: the schedule of ecsimd_msm_plan's bucket route."""
    if n == 0:
        return 1
    c = min(bits, min(16, max(2, n.bit_length() - 1 - 4)))
    windows = -(-bits // c)
    c = -(-bits // windows)
    m = min(1 << c, max(2, min(32, 1 << ((c + 1) // 2))))
    return 8 + tree_passes((1 << c) // m)


def test_the_launch_formula_restated_in_python(built):
    from ecsimd_amd import Engine
    for n in PLAN_SIZES:
        for bits in (128, 253):
            if n + (bits == 253) <= 1 << 24:
                assert Engine.ed25519_msm_plan(n + (bits == 253), bits)["launches"] == msm_launches(n + (bits == 253), bits), (n, bits)
        rc, p = plan(built, n, flags=MSM)
        levels = tree_passes(n)
        want = 1 if n == 0 else 5 + levels + max(1, levels) + msm_launches(n, 128) + msm_launches(n + 1, 253)
        assert rc == 0 and p.route == MSM and p.launches == want, (n, p.launches, want)
        rc, p = plan(built, n, flags=LANES | SMALL)
        assert rc == 0 and p.route == LANES and p.launches == (1 if n == 0 else 1 + 2 * ((n + (1 << 20) - 1) >> 20)), n
        assert Engine.ed25519_batch_plan(n, 32, MSM) == dict(route=MSM, launches=want, workspace_bytes=plan(built, n, flags=MSM)[1].workspace_bytes)
    t = threshold()
    if t > MAX_N:
        assert plan(built, MAX_N)[1].route == LANES                       # the MSM route never won its timing: AUTO is LANES everywhere
    else:
        assert plan(built, t - 1)[1].route == LANES and plan(built, t)[1].route == MSM and plan(built, MAX_N)[1].route == MSM


def test_workspace_bytes_is_monotone_in_n_and_the_schedule_is_ecsimd_msms(built):
    from ecsimd_amd import Engine
    for flags in (MSM, LANES):
        assert plan(built, 0, flags=flags)[1].workspace_bytes == 0
        last = 0
        sizes = sorted(set(range(1, 1200)) | {v for k in range(11, 25) for v in ((1 << k) - 2, (1 << k) - 1, 1 << k, (1 << k) + 1, 3 << (k - 1)) if v <= MAX_N})
        for n in sizes:
            w = plan(built, n, flags=flags)[1].workspace_bytes
            assert w >= last, (flags, n, w, last)
            last = w
            if flags == MSM:
                assert w >= max(Engine.ed25519_msm_plan(n, 128)["workspace_bytes"], Engine.ed25519_msm_plan(n + 1, 253)["workspace_bytes"]) + 32 * 7 * n      # h, leaf, z, z h, z s and the two term arrays
    assert [plan(built, 1000, m, MSM)[1].workspace_bytes for m in (0, 33, 1 << 20)] == [plan(built, 1000, 32, MSM)[1].workspace_bytes] * 3
    # the same schedule as ecsimd_msm's bucket route, field for field, and a workspace of its own: four planes, one plane fewer per term
    for n, bits in ((1, 1), (17, 4), (300, 253), (1 << 16, 256), (1 << 20, 128), (1 << 24, 256)):
        a, b = Engine.ed25519_msm_plan(n, bits), Engine.msm_plan(n, bits, 1)
        assert {k: v for k, v in a.items() if k != "workspace_bytes"} == {k: v for k, v in b.items() if k != "workspace_bytes"}, (n, bits)
        K, T = a["windows"] << a["c"], n * a["windows"]
        slices, lanes = -(-T // a["L"]), (a["buckets"] // a["m"]) * a["windows"]
        r16 = lambda v: (v + 15) // 16 * 16
        assert a["workspace_bytes"] == r16(16 + 4 * K) + r16(4 * (K + 1)) + r16(4 * K) + r16(4 * T) + 32 * (4 * n + 4 * K + 8 * slices + 4 * lanes), (n, bits)
        assert a["workspace_bytes"] - b["workspace_bytes"] == 32 * (n + K + 2 * slices + lanes), (n, bits)
    assert Engine.ed25519_msm_plan(0, 256) == dict(Engine.msm_plan(0, 256, 1), workspace_bytes=0)


def test_the_plans_refuse_what_the_calls_refuse(built):
    from ecsimd_amd import Engine, EcsimdHipError
    from ecsimd_amd.engine import MsmPlan
    assert plan(built, MAX_N)[0] == 0 and plan(built, MAX_N + 1)[0] == BAD_ARG
    for flags in (6, 7, 8, 3 | 8, 16, -1):
        assert plan(built, 8, flags=flags)[0] == BAD_ARG, flags
    for flags in (AUTO, MSM, LANES, AUTO | SMALL, MSM | SMALL, LANES | SMALL):
        assert plan(built, 8, flags=flags)[0] == 0, flags
    assert plan(built, 8, msg_bytes=(1 << 40) + 1)[0] == BAD_ARG and plan(built, 8, msg_bytes=1 << 40)[0] == 0
    assert built.ecsimd_ed25519_batch_plan(C.c_size_t(8), C.c_size_t(32), C.c_int(0), None) == BAD_ARG
    with pytest.raises(EcsimdHipError):
        Engine.ed25519_batch_plan(MAX_N + 1, 32)
    p = MsmPlan()
    msm_plan = lambda n, bits, flags, out=C.byref(p): built.ecsimd_ed25519_msm_plan(C.c_size_t(n), C.c_int(bits), C.c_int(flags), out)
    assert msm_plan(1 << 24, 256, 0) == 0 and msm_plan((1 << 24) + 1, 256, 0) == BAD_ARG
    assert msm_plan(8, 0, 0) == BAD_ARG and msm_plan(8, 257, 0) == BAD_ARG and msm_plan(8, 1, 1) == 0
    assert msm_plan(8, 256, 2) == BAD_ARG and msm_plan(8, 256, 3) == BAD_ARG and msm_plan(8, 256, -1) == BAD_ARG      # LANES is ecsimd_msm's, not this call's
    assert msm_plan(8, 256, 0, None) == BAD_ARG
    with pytest.raises(EcsimdHipError):
        Engine.ed25519_msm_plan(8, 256, 2)
    # no context: the calls refuse before they touch anything
    z = C.c_size_t(0)
    assert built.ecsimd_ed25519_verify_batch(None, None, None, z, z, None, None, None, z, C.c_int(0)) == BAD_ARG
    assert built.ecsimd_ed25519_verify_cofactored(None, None, None, z, z, None, None, None, z, C.c_int(0)) == BAD_ARG
    assert built.ecsimd_ed25519_batch_randomizers(None, None, None, z, z, None, None, None, z) == BAD_ARG
    assert built.ecsimd_ed25519_msm(None, None, None, None, None, None, z, C.c_int(256), C.c_int(0)) == BAD_ARG


# ---- the boundary
def test_the_header_is_c99_and_a_caller_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_ed25519_batch.h"
#include <stddef.h>
int main(int argc, char** argv) {
  ecsimd_ed25519_batch_plan_t p; ecsimd_msm_plan_t m;
  uint8_t* b = NULL; const uint32_t* lens = NULL; uint32_t* inv = NULL; (void)argv;
  if (ecsimd_ed25519_batch_plan(17, 32, ECSIMD_ED25519_BATCH_MSM | ECSIMD_ED25519_REJECT_SMALL_ORDER, &p) != ECSIMD_HIP_OK || p.route != ECSIMD_ED25519_BATCH_MSM || p.launches < 10) return 1;
  if (ecsimd_ed25519_batch_plan(ECSIMD_MSM_MAX_N, 32, ECSIMD_ED25519_BATCH_AUTO, &p) != ECSIMD_HIP_ERR_BAD_ARG) return 2;
  if (ECSIMD_ED25519_BATCH_AUTO_THRESHOLD < 2) return 3;
  if (ecsimd_ed25519_msm_plan(300, 253, ECSIMD_MSM_ALG_BUCKETS, &m) != ECSIMD_HIP_OK || m.route != ECSIMD_MSM_ALG_BUCKETS || m.L != 8) return 4;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_ed25519_verify_batch(NULL, b, b, 32, 32, lens, b, b, 0, ECSIMD_ED25519_BATCH_LANES);
    rc |= ecsimd_ed25519_verify_cofactored(NULL, b, b, 32, 32, lens, b, b, 0, 0);
    rc |= ecsimd_ed25519_batch_randomizers(NULL, b, b, 32, 40, lens, b, b, 0);
    rc |= ecsimd_ed25519_msm(NULL, b, b, b, b, inv, 0, 253, 0);
    return rc;
  }
  return 0;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    assert subprocess.run([str(exe)]).returncode == 0          # the plans are host only: they run here


def test_the_names_are_exported_and_the_bindings_exist(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", out, re.M))
    for name in NAMES:
        assert name in exported and hasattr(built, name), name
    assert sorted(s for s in exported if s.startswith("ecsimd_hip_")) == declared_symbols()
    text = open(HEADER).read()
    assert re.findall(r"\b(ecsimd_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)) == list(NAMES)
    assert "NOT ZIP-215" in text and "DETERMINISM" in text and "SOUNDNESS" in text
    assert "does not exist here" not in open(os.path.join(ROOT, "include", "ecsimd_ed25519.h")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_msm_ed25519.hip" in mk and "ecsimd_ed25519_batch.h" in mk
    from ecsimd_amd import Engine, flags
    assert (flags.ED25519_BATCH_AUTO, flags.ED25519_BATCH_MSM, flags.ED25519_BATCH_LANES, flags.ED25519_REJECT_SMALL_ORDER) == (AUTO, MSM, LANES, SMALL)
    for m in ("ed25519_msm", "ed25519_msm_plan", "ed25519_verify_cofactored", "ed25519_verify_batch", "ed25519_batch_randomizers", "ed25519_batch_plan"):
        assert callable(getattr(Engine, m)), m


def test_no_kernel_of_the_new_unit_spills_and_the_listing_file_is_the_builds(built):
    """profiles/r17/ed25519_batch_listing.json against the ISA the build left: VGPRs and scratch per kernel, no spill, 256-thread workgroups."""
    isa = os.path.join(ROOT, "build", "csrc", "k_msm_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.getmtime(isa) >= os.path.getmtime(os.path.join(CSRC, "k_msm_ed25519.hip"))
    text = open(isa).read()
    got = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = re.search(r"(k_ed[mbc]_[a-z]+)", name).group(1)
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        got[short] = dict(vgprs=field("vgpr_count"), scratch_bytes=field("private_segment_fixed_size"), vgpr_spills=field("vgpr_spill_count"),
                          max_workgroup=field("max_flat_workgroup_size"))
    assert len(got) == 14, sorted(got)
    for k, v in got.items():
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0, (k, v)
        assert v["max_workgroup"] == (64 if k in ("k_edm_final", "k_edb_seed", "k_edb_accept") else 256), (k, v)
    listing = json.load(open(os.path.join(ROOT, "profiles", "r17", "ed25519_batch_listing.json")))
    assert listing["kernels"] == {k: dict(vgprs=v["vgprs"], scratch_bytes=v["scratch_bytes"]) for k, v in got.items()}
    head = open(os.path.join(CSRC, "k_msm_ed25519.hip")).read().split("#include")[0]
    for k, v in got.items():
        assert "%s %d / %d" % (k, v["vgprs"], v["scratch_bytes"]) in head, k
