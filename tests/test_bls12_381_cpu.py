"""BLS12-381 G1, the part that needs no GPU: the model the GPU tests take their expected values from (tools/bls12_381_model.py) asserts the curve facts and
regenerates the committed fixture byte for byte; fe381.cuh / g1.cuh, compiled for the HOST, equal Python integers and the model on the representation's bounds,
on every exceptional pair of the group law (a hand-made Y = 0 included), on the scalar product, the subgroup test and both encodings with every kind of
malformed record; ecsimd_bls12_381_g1_msm_plan equals the model's restatement of the schedule; and ecsimd_msm_plan / ecsimd_ed25519_msm_plan still report, field
for field, what the commit before this feature reported."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_381_model as model      # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_bls12_381.h")
SYMBOLS = {"ecsimd_bls12_381_" + s for s in ("g1_decompress", "g1_compress", "g1_check", "g1_mul", "g1_msm", "g1_point_sum", "g1_msm_plan", "raw", "raw_inputs", "raw_outputs")}
P, R, G, INF = model.P, model.R, model.G, model.INF
ALL = 2**384 - 1
NS, BITS = (0, 1, 2, 17, 1000, 4097, 2**20), (1, 128, 255, 256)
FIELDS = ("route", "c", "windows", "buckets", "L", "m", "max_chain", "launches", "workspace_bytes")


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=3000)
    return ecsimd_amd.load_library()


# ---- the model and the fixture
def test_the_model_asserts_the_curve_facts():
    model._self_check()
    assert model.is_prime(P) and model.is_prime(R) and not model.is_prime(P * R) and not model.is_prime(model.H)
    assert model.mul(R, G) is INF and model.add(G, G)[0] == model.X2_2G and model.encode48(G)[0] == 0x97
    assert model.H * R == P + 1 - (model.X + 1)
    q = model.curve_point(5)
    assert model.on_curve(q) and model.mul(model.H * R, q) is INF                                 # the curve's order kills every point of E(Fp)
    assert model.in_subgroup(model.mul(model.H, q))                                              # clearing the cofactor lands in G1


def test_the_endomorphism_test_equals_the_definition_on_the_fixture():
    fx = json.load(open(model.FIXTURE))
    recs = fx["multiples"] + fx["off_subgroup"] + [fx["h_torsion"]]
    assert sum(1 for r in recs if not r["in_subgroup"]) >= 5
    for r in recs:
        pt = model.decode96(bytes.fromhex(r["uncompressed"]))
        assert model.in_subgroup(pt) == model.endo_in_subgroup(pt) == r["in_subgroup"]


def test_the_fixture_regenerates_byte_for_byte_and_stays_small():
    stored = open(model.FIXTURE).read()
    assert stored == model.fixture_text()
    fx = json.loads(stored)
    assert len(stored) < 64 * 1024 and len(fx["multiples"]) >= 16 and len(fx["malformed_uncompressed"]) >= 10 and len(fx["malformed_compressed"]) >= 7
    assert fx["multiples"][0]["uncompressed"] == "40" + "00" * 95 and fx["multiples"][0]["compressed"] == "c0" + "00" * 47
    assert {bool(bytes.fromhex(m["compressed"])[0] & 0x20) for m in fx["multiples"][1:]} == {True, False}   # both signs of y
    for want in (0, 1, P - 1, P, ALL):
        assert "%096x" % want in fx["field_operands"]


def test_the_model_refuses_every_malformed_record_and_round_trips_the_rest():
    fx = json.load(open(model.FIXTURE))
    for m in fx["malformed_uncompressed"]:
        assert model.decode96(bytes.fromhex(m["bytes"])) is model.MALFORMED, m["why"]
    for m in fx["malformed_compressed"]:
        assert model.decode48(bytes.fromhex(m["bytes"])) is model.MALFORMED, m["why"]
    for m in fx["multiples"]:
        pt = model.mul(int(m["k"], 16), G)
        assert model.encode96(pt).hex() == m["uncompressed"] and model.encode48(pt).hex() == m["compressed"]
        assert model.decode96(bytes.fromhex(m["uncompressed"])) == pt and model.decode48(bytes.fromhex(m["compressed"])) == pt


def test_the_msm_is_the_plain_sum():
    rng = random.Random(2)
    a0, d = rng.randrange(R), rng.randrange(R)
    pts, acc, step = [], model.mul(a0, G), model.mul(d, G)
    for _ in range(9):
        pts.append(acc); acc = model.add(acc, step)
    ks = [rng.getrandbits(256) for _ in pts]
    assert model.msm(ks, pts) == model.mul(sum(k * (a0 + i * d) for i, k in enumerate(ks)) % R, G)
    assert model.msm(ks, pts, bits=7) == model.mul(sum((k % 128) * (a0 + i * d) for i, k in enumerate(ks)) % R, G)


# ---- the device layers on the host
def test_the_field_the_group_law_and_the_encodings_on_the_host(tmp_path):
    exe = tmp_path / "bls12_381_host_check"
    subprocess.run(["hipcc", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "bls12_381_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=1200)
    fx = json.load(open(model.FIXTURE))
    rng = random.Random(381)
    h = lambda v: "%096x" % v
    reqs, exps = [], []
    pt3 = lambda p: [0, 0, 1] if p is INF else [p[0], p[1], 0]

    def ask(op, args, exp):
        reqs.append(op + " " + " ".join(h(a) for a in args)); exps.append(list(exp))
    bounds = [int(v, 16) for v in fx["field_operands"]]
    ops = bounds + [0xffffffff << (32 * j) for j in range(12)] + [ALL ^ (0xffffffff << (32 * j)) for j in range(12)]
    pairs = [(a, b) for a in bounds for b in bounds] + [(a, a) for a in ops] + [(a, rng.getrandbits(384)) for a in ops] + [(rng.getrandbits(384), rng.getrandbits(384)) for _ in range(200)]
    for a, b in pairs:
        ask("mul", [a, b], [a * b % P]); ask("add", [a, b], [(a + b) % P]); ask("sub", [a, b], [(a - b) % P])
    for a in ops + [rng.getrandbits(384) for _ in range(50)]:
        ask("sqr", [a], [a * a % P]); ask("neg", [a], [-a % P]); ask("canon", [a], [a % P]); ask("lex", [a], [1 if a % P > (P - 1) // 2 else 0])
    for a in bounds + [rng.getrandbits(384) for _ in range(4)]:
        ask("inv", [a], [pow(a, P - 2, P)])
    for a in [0, 1, 4, P - 1, P, ALL] + [rng.getrandbits(384) for _ in range(12)]:
        s = model.fe_sqrt(a)
        ask("sqrt", [a], [pow(a, (P + 1) // 4, P), 0 if s is None else 1])
    off = [model.decode96(bytes.fromhex(r["uncompressed"])) for r in fx["off_subgroup"]]
    tors = model.decode96(bytes.fromhex(fx["h_torsion"]["uncompressed"]))
    pts = [INF, G, model.neg(G), model.add(G, G), off[0], tors] + [model.mul(rng.randrange(R), G) for _ in range(3)]
    for a in pts:
        ask("pdbl", pt3(a), pt3(model.add(a, a)))
        for b in pts:
            ask("padd", pt3(a) + pt3(b), pt3(model.add(a, b)))                                      # generic, P + P, P + (-P), either and both at infinity
            if b is not INF:
                ask("pmadd", pt3(a) + list(b), pt3(model.add(a, b)))
    ask("jdbl", [5, 0, 1], [0, 0, 1])                                                              # Y = 0: the curve has no such point; the double is the identity all the same
    ask("jdbl", [G[0], G[1], 0], [0, 0, 1])                                                        # Z = 0
    z = rng.randrange(1, P)
    ask("jdbl", [G[0] * z * z % P, G[1] * z ** 3 % P, z], pt3(model.add(G, G)))
    ks = [0, 1, 2, 15, 16, R - 1, R, R + 1, 2**256 - 1, 2**255, int("8" * 64, 16), int("7" * 64, 16)] + [rng.getrandbits(256) for _ in range(6)]
    for k in ks:
        for pt in (G, pts[-1], off[1]):
            ask("pmul", [k, pt[0], pt[1]], pt3(model.mul(k, pt)))                                   # integer semantics: off[1] is not in G1
    for pt in [G, pts[-1], pts[-2], tors] + off:
        ask("subgroup", [0, pt[0], pt[1]], [1 if model.in_subgroup(pt) else 0])
    words = lambda b: int.from_bytes(b, "big")
    cls_of = lambda pt: (2, 0, 0) if pt is model.MALFORMED else (0, 0, 0) if pt is INF else (1, pt[0], pt[1])
    for r in fx["multiples"] + fx["off_subgroup"] + [fx["h_torsion"]]:
        u, c = bytes.fromhex(r["uncompressed"]), bytes.fromhex(r["compressed"])
        pt = model.decode96(u)
        ask("dec96", [words(u[:48]), words(u[48:])], cls_of(pt)); ask("dec48", [words(c)], cls_of(pt))
        ask("enc", pt3(pt)[2:] + pt3(pt)[:2], [words(u[:48]), words(u[48:]), words(c)])
    for m in fx["malformed_uncompressed"]:
        u = bytes.fromhex(m["bytes"])
        ask("dec96", [words(u[:48]), words(u[48:])], [2, 0, 0])
    for m in fx["malformed_compressed"]:
        ask("dec48", [words(bytes.fromhex(m["bytes"]))], [2, 0, 0])
    out = subprocess.run([str(exe)], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=900)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == len(reqs), out.stderr[-500:]
    wrong = [(r[:90], l[:200]) for r, e, l in zip(reqs, exps, lines) if [int(x, 16) for x in l.split()] != e]
    assert not wrong, wrong[:5]


# ---- the C ABI and the plans
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols, declared_bls12_381_symbols
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_bls12_381_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(declared_bls12_381_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_bls12_381")} == declared
    hip = {s for s in exported if s.startswith("ecsimd_hip_")}
    assert hip == set(declared_symbols())                                                        # no new ecsimd_hip_* symbol
    assert "PUBLIC DATA ONLY" in text and "g1_check" in text and '#include "ecsimd_msm.h"' in text
    from ecsimd_amd import Engine
    for m in ("g1_decompress", "g1_compress", "g1_check", "g1_mul", "g1_msm", "g1_point_sum", "g1_msm_plan", "raw"):
        assert callable(getattr(Engine, "bls12_381_" + m)), m
    ins, outs = (2, 1, 2, 2, 1, 1, 1, 1, 6, 3, 5), (1, 1, 1, 1, 1, 1, 2, 1, 3, 3, 3)
    assert tuple(built.ecsimd_bls12_381_raw_inputs(op) for op in range(11)) == ins and tuple(built.ecsimd_bls12_381_raw_outputs(op) for op in range(11)) == outs
    for fn in (built.ecsimd_bls12_381_raw_inputs, built.ecsimd_bls12_381_raw_outputs):
        assert fn(-1) == 0 and fn(11) == 0


def plan_of(lib, name, n, bits, flags):
    from ecsimd_amd.engine import MsmPlan
    p = MsmPlan()
    rc = getattr(lib, name)(C.c_size_t(n), C.c_int(bits), C.c_int(flags), C.byref(p))
    return None if rc != 0 else {f: int(getattr(p, f)) for f in FIELDS}


def threshold():
    m = re.search(r"#define ECSIMD_BLS12_381_MSM_AUTO_THRESHOLD \(\(size_t\)1 << (\d+)\)", open(HEADER).read())
    return 1 << int(m.group(1))


def test_g1_msm_plan_is_the_models_restatement_of_the_schedule(built):
    built.ecsimd_bls12_381_g1_msm_plan.restype = C.c_int
    th = threshold()
    for n in NS + (th - 1, th, 2**24):
        for bits in BITS:
            for flags in (0, 1, 2):
                assert plan_of(built, "ecsimd_bls12_381_g1_msm_plan", n, bits, flags) == model.plan(n, bits, flags, th), (n, bits, flags)
    for n, bits, flags in ((1, 0, 0), (1, 257, 0), (2**24 + 1, 255, 0), (1, 255, 3), (1, 255, -1)):
        assert plan_of(built, "ecsimd_bls12_381_g1_msm_plan", n, bits, flags) is None and model.plan(n, bits, flags, th) is None
    assert built.ecsimd_bls12_381_g1_msm_plan(C.c_size_t(1), C.c_int(255), C.c_int(0), None) != 0
    a, b = plan_of(built, "ecsimd_bls12_381_g1_msm_plan", 4097, 255, 1), plan_of(built, "ecsimd_msm_plan", 4097, 255, 1)
    assert {f: a[f] for f in FIELDS[:-1]} == {f: b[f] for f in FIELDS[:-1]} and a["workspace_bytes"] > b["workspace_bytes"]   # one schedule, wider elements


# What ecsimd_msm_plan (BUCKETS, LANES) and ecsimd_ed25519_msm_plan (BUCKETS) reported at the commit before this feature, read from its build:
# (n, bits) -> (c, windows, buckets, L, m, max_chain, launches, workspace_bytes) for BUCKETS; LANES has no c .. m.
PARENT_MSM_BUCKETS = {
    (0, 1): (0, 0, 0, 0, 0, 0, 1, 0), (0, 128): (0, 0, 0, 0, 0, 0, 1, 0), (0, 255): (0, 0, 0, 0, 0, 0, 1, 0), (0, 256): (0, 0, 0, 0, 0, 0, 1, 0),
    (1, 1): (1, 1, 2, 4, 2, 16, 8, 656), (1, 128): (2, 64, 4, 4, 2, 192, 9, 43392), (1, 255): (2, 128, 4, 4, 2, 384, 9, 86656), (1, 256): (2, 128, 4, 4, 2, 384, 9, 86656),
    (2, 1): (1, 1, 2, 4, 2, 16, 8, 752), (2, 128): (2, 64, 4, 4, 2, 192, 9, 46816), (2, 255): (2, 128, 4, 4, 2, 384, 9, 93408), (2, 256): (2, 128, 4, 4, 2, 384, 9, 93408),
    (17, 1): (1, 1, 2, 4, 2, 16, 8, 3024), (17, 128): (2, 64, 4, 4, 2, 192, 9, 98176), (17, 255): (2, 128, 4, 4, 2, 384, 9, 194688), (17, 256): (2, 128, 4, 4, 2, 384, 9, 194688),
    (1000, 1): (1, 1, 2, 8, 2, 126, 8, 124352), (1000, 128): (5, 26, 32, 8, 8, 156, 9, 923872), (1000, 255): (5, 51, 32, 8, 8, 306, 9, 1719872), (1000, 256): (5, 52, 32, 8, 8, 312, 9, 1751712),
    (4097, 1): (1, 1, 2, 32, 2, 130, 8, 434832), (4097, 128): (8, 16, 256, 32, 16, 144, 9, 1515904), (4097, 255): (8, 32, 256, 32, 16, 288, 9, 2638272), (4097, 256): (8, 32, 256, 32, 16, 288, 9, 2638272),
    (1048576, 1): (1, 1, 2, 256, 2, 4097, 8, 105644384), (1048576, 128): (16, 8, 65536, 256, 32, 4097, 11, 198705184), (1048576, 255): (16, 16, 65536, 256, 32, 4097, 11, 296747040), (1048576, 256): (16, 16, 65536, 256, 32, 4097, 11, 296747040),
}
PARENT_MSM_LANES = {
    (0, 1): (0, 0, 0, 0, 0, 0, 1, 0), (0, 128): (0, 0, 0, 0, 0, 0, 1, 0), (0, 255): (0, 0, 0, 0, 0, 0, 1, 0), (0, 256): (0, 0, 0, 0, 0, 0, 1, 0),
    (1, 1): (0, 0, 0, 0, 0, 16, 9, 1696), (1, 128): (0, 0, 0, 0, 0, 16, 9, 1696), (1, 255): (0, 0, 0, 0, 0, 16, 9, 1696), (1, 256): (0, 0, 0, 0, 0, 16, 9, 1696),
    (2, 1): (0, 0, 0, 0, 0, 16, 9, 3264), (2, 128): (0, 0, 0, 0, 0, 16, 9, 3264), (2, 255): (0, 0, 0, 0, 0, 16, 9, 3264), (2, 256): (0, 0, 0, 0, 0, 16, 9, 3264),
    (17, 1): (0, 0, 0, 0, 0, 16, 10, 26880), (17, 128): (0, 0, 0, 0, 0, 16, 10, 26880), (17, 255): (0, 0, 0, 0, 0, 16, 10, 26880), (17, 256): (0, 0, 0, 0, 0, 16, 10, 26880),
    (1000, 1): (0, 0, 0, 0, 0, 16, 11, 1574080), (1000, 128): (0, 0, 0, 0, 0, 16, 11, 1574080), (1000, 255): (0, 0, 0, 0, 0, 16, 11, 1574080), (1000, 256): (0, 0, 0, 0, 0, 16, 11, 1574080),
    (4097, 1): (0, 0, 0, 0, 0, 16, 12, 6448800), (4097, 128): (0, 0, 0, 0, 0, 16, 12, 6448800), (4097, 255): (0, 0, 0, 0, 0, 16, 12, 6448800), (4097, 256): (0, 0, 0, 0, 0, 16, 12, 6448800),
    (1048576, 1): (0, 0, 0, 0, 0, 16, 13, 1650458656), (1048576, 128): (0, 0, 0, 0, 0, 16, 13, 1650458656), (1048576, 255): (0, 0, 0, 0, 0, 16, 13, 1650458656), (1048576, 256): (0, 0, 0, 0, 0, 16, 13, 1650458656),
}
PARENT_ED25519_BUCKETS = {
    (0, 1): (0, 0, 0, 0, 0, 0, 1, 0), (0, 128): (0, 0, 0, 0, 0, 0, 1, 0), (0, 255): (0, 0, 0, 0, 0, 0, 1, 0), (0, 256): (0, 0, 0, 0, 0, 0, 1, 0),
    (1, 1): (1, 1, 2, 4, 2, 16, 8, 848), (1, 128): (2, 64, 4, 4, 2, 192, 9, 56736), (1, 255): (2, 128, 4, 4, 2, 384, 9, 113312), (1, 256): (2, 128, 4, 4, 2, 384, 9, 113312),
    (2, 1): (1, 1, 2, 4, 2, 16, 8, 976), (2, 128): (2, 64, 4, 4, 2, 192, 9, 61216), (2, 255): (2, 128, 4, 4, 2, 384, 9, 122144), (2, 256): (2, 128, 4, 4, 2, 384, 9, 122144),
    (17, 1): (1, 1, 2, 4, 2, 16, 8, 3984), (17, 128): (2, 64, 4, 4, 2, 192, 9, 128416), (17, 255): (2, 128, 4, 4, 2, 384, 9, 254624), (17, 256): (2, 128, 4, 4, 2, 384, 9, 254624),
    (1000, 1): (1, 1, 2, 8, 2, 126, 8, 164448), (1000, 128): (5, 26, 32, 8, 8, 156, 9, 1193824), (1000, 255): (5, 51, 32, 8, 8, 306, 9, 2218624), (1000, 256): (5, 52, 32, 8, 8, 312, 9, 2259616),
    (4097, 1): (1, 1, 2, 32, 2, 130, 8, 574288), (4097, 128): (8, 16, 256, 32, 16, 144, 9, 1917408), (4097, 255): (8, 32, 256, 32, 16, 288, 9, 3310112), (4097, 256): (8, 32, 256, 32, 16, 288, 9, 3310112),
    (1048576, 1): (1, 1, 2, 256, 2, 4097, 8, 139461056), (1048576, 128): (16, 8, 65536, 256, 32, 4097, 11, 251658272), (1048576, 255): (16, 16, 65536, 256, 32, 4097, 11, 369098784), (1048576, 256): (16, 16, 65536, 256, 32, 4097, 11, 369098784),
}


def test_the_old_callers_plans_are_what_the_parent_commit_reported(built):
    assert len(PARENT_MSM_BUCKETS) == len(PARENT_MSM_LANES) == len(PARENT_ED25519_BUCKETS) == len(NS) * len(BITS)
    for n in NS:
        for bits in BITS:
            for name, flags, table in (("ecsimd_msm_plan", 1, PARENT_MSM_BUCKETS), ("ecsimd_msm_plan", 2, PARENT_MSM_LANES), ("ecsimd_ed25519_msm_plan", 1, PARENT_ED25519_BUCKETS)):
                p = plan_of(built, name, n, bits, flags)
                assert p["route"] == flags and tuple(p[f] for f in FIELDS[1:]) == table[(n, bits)], (name, n, bits)
            auto = plan_of(built, "ecsimd_msm_plan", n, bits, 0)
            assert auto == plan_of(built, "ecsimd_msm_plan", n, bits, 1 if n >= 2**20 else 2)


def test_the_shipped_listing_has_the_figures_the_profile_records(built):
    """tools/bls12_381_listing.py --unit g1 --check on the listing the build left in build/csrc, and, said per figure, what no change of the unit may move
    unnoticed: every kernel's instruction counts, registers, scratch and spills.  Kernel names, resource lines and instruction counts only."""
    import bls12_381_listing as listing
    path = os.path.join(ROOT, "build", "csrc", listing.UNITS["g1"]["listing"] + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_bls12_381.hip", "k_bls12_381.inc", "bls381_curve.inc", "g1.cuh", "fe381.cuh", "fe384.cuh", "bls381_bytes.cuh", "msm_stages.cuh", "kernels.h"):
        assert os.path.getmtime(path) >= os.path.getmtime(os.path.join(CSRC, f)), f
    got, recorded = listing.report("g1"), json.load(open(os.path.join(ROOT, listing.UNITS["g1"]["out"])))
    assert len(recorded["kernels"]) == 14
    for section in ("kernels", "functions"):
        for name, figures in recorded.get(section, {}).items():
            for f in ("valu", "mads", "registers", "agprs", "vgprs", "private_segment_fixed_size", "scratch_bytes", "vgpr_spill_count", "text_bytes"):
                if f in figures:
                    assert got[section][name][f] == figures[f], (name, f, got[section][name][f], figures[f])
    assert got == recorded, f"{listing.UNITS['g1']['out']} is stale: python tools/bls12_381_listing.py --unit g1"
