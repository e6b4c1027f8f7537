"""BLS12-381 G2, the part that needs no GPU: the model the GPU tests take their expected values from (tools/bls12_381_g2_model.py) asserts the curve facts, holds
the psi subgroup test to the definition on the fixture and regenerates the committed fixture byte for byte; fp2.cuh / g2.cuh, compiled for the HOST, equal Python
integers and the model on the representation's bounds in both components, on square roots of every class, on every exceptional pair of the group law (hand-made
Y = 0 and Z = 0 included), on the scalar product, the subgroup test and all four codecs with every kind of malformed record; the new header declares exactly the
new names and the library exports exactly those; ecsimd_bls381_g2_msm_plan equals the model's restatement of the schedule."""
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
import bls12_381_g2_model as model      # noqa: E402
import bls12_381_model as g1_model      # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_bls12_381_g2.h")
NAMES = ("decompress", "compress", "check", "mul", "msm", "point_sum", "msm_plan", "raw", "raw_inputs", "raw_outputs")
SYMBOLS = {"ecsimd_bls381_g2_" + s for s in NAMES}
G1_SYMBOLS = {"ecsimd_bls12_381_" + s for s in ("g1_decompress", "g1_compress", "g1_check", "g1_mul", "g1_msm", "g1_point_sum", "g1_msm_plan", "raw", "raw_inputs", "raw_outputs")}
P, R, G, INF = model.P, model.R, model.G, model.INF
ALL = 2**384 - 1
NS, BITS = (0, 1, 2, 17, 1000, 4097, 2**20), (1, 128, 255, 256)
FIELDS = ("route", "c", "windows", "buckets", "L", "m", "max_chain", "launches", "workspace_bytes")


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=3000)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def fx():
    return json.load(open(model.FIXTURE))


# ---- the model and the fixture
def test_the_model_asserts_the_curve_facts_and_psi_equals_the_definition_on_the_fixture(fx):
    recs = model.point_records(fx)
    assert sum(1 for r in recs if not r["in_subgroup"]) >= 5
    model._self_check(recs)
    assert model.H2.bit_length() == 507 and model.H2 % 2 == 1 and model.encode96(G)[0] == 0x93
    assert model.mul(R, G) is INF and model.decode96(model.encode96(G)) == G
    assert fx["cofactor_cleared"]["in_subgroup"] and not fx["h_torsion"]["in_subgroup"]
    assert not any(r["in_subgroup"] for r in fx["off_subgroup"]) and len(fx["off_subgroup"]) >= 4


def test_the_fixture_regenerates_byte_for_byte_and_stays_small(fx):
    stored = open(model.FIXTURE).read()
    assert stored == model.fixture_text()
    assert len(stored) < 64 * 1024 and len(fx["multiples"]) >= 16
    ks = {int(m["k"], 16) for m in fx["multiples"]}
    assert {0, 1, 2, R - 1} <= ks
    assert fx["multiples"][0]["uncompressed"] == "40" + "00" * 191 and fx["multiples"][0]["compressed"] == "c0" + "00" * 95
    assert {bool(bytes.fromhex(m["compressed"])[0] & 0x20) for m in fx["multiples"][1:]} == {True, False}   # both values of the sort bit
    real, imag = model.decode192(bytes.fromhex(fx["real_y"]["uncompressed"])), model.decode192(bytes.fromhex(fx["imaginary_y"]["uncompressed"]))
    assert real[1][1] == 0 and real[1][0] != 0 and imag[1][0] == 0 and imag[1][1] != 0
    assert {bool(bytes.fromhex(fx[k]["compressed"])[0] & 0x20) for k in ("real_y", "real_y_negated")} == {True, False}       # the tie-break on c1 = 0 decides
    for want in (0, 1, P - 1, P, ALL):
        assert "%096x" % want in fx["field_operands"]
    whys = " ".join(m["why"] for m in fx["malformed_uncompressed"])
    for name in ("x.c1", "x.c0", "y.c1", "y.c0"):
        assert name + " is p" in whys and name + " off by one" in whys and "a byte in " + name in whys
    whys = " ".join(m["why"] for m in fx["malformed_compressed"])
    for name in ("x.c1 is p", "x.c0 is p", "sort bit", "a byte in x.c1", "a byte in x.c0", "no square root", "bit 7 clear"):
        assert name in whys


def test_the_model_refuses_every_malformed_record_and_round_trips_the_rest(fx):
    for m in fx["malformed_uncompressed"]:
        assert model.decode192(bytes.fromhex(m["bytes"])) is model.MALFORMED, m["why"]
    for m in fx["malformed_compressed"]:
        assert model.decode96(bytes.fromhex(m["bytes"])) is model.MALFORMED, m["why"]
    for m in fx["multiples"]:
        pt = model.mul(int(m["k"], 16), G)
        assert model.encode192(pt).hex() == m["uncompressed"] and model.encode96(pt).hex() == m["compressed"]
    for m in model.point_records(fx):
        pt = model.decode192(bytes.fromhex(m["uncompressed"]))
        assert pt is not model.MALFORMED and model.on_curve(pt) and model.decode96(bytes.fromhex(m["compressed"])) == pt
        assert model.encode192(pt).hex() == m["uncompressed"] and model.encode96(pt).hex() == m["compressed"]


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
def test_the_field_the_group_law_and_the_encodings_on_the_host(tmp_path, fx):
    exe = tmp_path / "bls12_381_g2_host_check"
    subprocess.run(["hipcc", "--offload-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "bls12_381_g2_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, timeout=1200)
    rng = random.Random(3812)
    h = lambda v: "%096x" % v
    reqs, exps, checks = [], [], []
    red = lambda a: (a[0] % P, a[1] % P)
    pt5 = lambda p: [0, 0, 0, 0, 1] if p is INF else [p[0][0], p[0][1], p[1][0], p[1][1], 0]
    rnd2 = lambda: (rng.getrandbits(384), rng.getrandbits(384))

    def ask(op, args, exp, check=None):
        reqs.append(op + " " + " ".join(h(a) for a in args)); exps.append(None if exp is None else list(exp)); checks.append(check)
    bounds = [int(v, 16) for v in fx["field_operands"]]
    key = [0, 1, P - 1, P, ALL]
    elems = [(a, b) for a in key for b in key]                                                      # the bounds in both components
    words = [(0xffffffff << (32 * j), 0) for j in range(12)] + [(0, 0xffffffff << (32 * j)) for j in range(12)] + [(ALL ^ (0xffffffff << (32 * j)), 1 << (32 * j)) for j in range(12)]
    pairs = [(a, b) for a in elems for b in elems] + [(a, a) for a in words] + [(a, rnd2()) for a in words] + [((a, b), (b, a)) for a in bounds for b in bounds[:5]] \
        + [(rnd2(), rnd2()) for _ in range(200)]
    for a, b in pairs:
        ask("mul", a + b, model.f2_mul(a, b)); ask("add", a + b, model.f2_add(a, b)); ask("sub", a + b, model.f2_sub(a, b))
        ask("eq", a + b, [1 if red(a) == red(b) else 0])
    singles = elems + words + [(a, b) for a in bounds for b in (0, 1, P - 1)] + [rnd2() for _ in range(50)]
    for a in singles:
        ask("sqr", a, model.f2_sqr(a)); ask("neg", a, model.f2_neg(a)); ask("conj", a, model.f2_conj(a)); ask("canon", a, red(a))
        ask("dbl", a, model.f2_add(a, a)); ask("iszero", a, [1 if red(a) == (0, 0) else 0])
        ask("lex", a, [1 if model.lex_largest(a) else 0])                                           # c1 = 0 among them: the tie-break
    for a in elems + [rnd2() for _ in range(6)]:
        inv = model.f2_inv(a)
        assert red(a) == (0, 0) and inv == (0, 0) or model.f2_mul(a, inv) == (1, 0)
        ask("inv", a, inv)

    def root_check(a):
        a = red(a)
        have = model.f2_sqrt(a) is not None
        def check(got):                                                                             # a root whenever one exists, the flag true exactly then
            return got[2] == (1 if have else 0) and (not have or model.f2_sqr((got[0], got[1])) == a)
        return check
    qr = [v for v in range(2, 40) if g1_model.fe_sqrt(v) is not None][:4]
    nqr = [v for v in range(2, 40) if g1_model.fe_sqrt(v) is None][:4]
    assert len(qr) == 4 and len(nqr) == 4
    in_fp = [(0, 0), (1, 0), (P - 1, 0), (P, P), (ALL, 0)] + [(v, 0) for v in qr + nqr] + [(rng.randrange(P), 0) for _ in range(6)]
    squares = [model.f2_sqr(rnd2()) for _ in range(8)] + [(0, v) for v in (1, 2, P - 1)]
    nonsquares = []
    while len(nonsquares) < 8:
        a = red(rnd2())
        if model.f2_sqrt(a) is None:
            nonsquares.append(a)
    for a in in_fp:
        assert model.f2_sqrt(a) is not None                                                         # every element of Fp has a root in Fp2
    for a in in_fp + squares + nonsquares + [rnd2() for _ in range(8)]:
        ask("sqrt", a, None, root_check(a))
    for v in qr:                                                                                     # a residue of Fp: the real root; a non-residue: the purely imaginary one
        ask("sqrt", (v, 0), None, lambda got, v=v: got[1] == 0 and got[0] * got[0] % P == v and got[2] == 1)
    for v in nqr:
        ask("sqrt", (v, 0), None, lambda got, v=v: got[0] == 0 and (-got[1] * got[1]) % P == v and got[2] == 1)

    dec = lambda r: model.decode192(bytes.fromhex(r["uncompressed"]))
    off = [dec(r) for r in fx["off_subgroup"]]
    tors = dec(fx["h_torsion"])
    pts = [INF, G, model.neg(G), model.add(G, G), off[0], tors] + [model.mul(rng.randrange(R), G) for _ in range(3)]
    for a in pts:
        ask("pdbl", pt5(a), pt5(model.add(a, a)))
        for b in pts:
            ask("padd", pt5(a) + pt5(b), pt5(model.add(a, b)))                                      # generic, P + P, P + (-P), either and both at infinity
            if b is not INF:
                ask("pmadd", pt5(a) + pt5(b)[:4], pt5(model.add(a, b)))
    ask("jdbl", [5, 7, 0, 0, 1, 0], [0, 0, 0, 0, 1])                                                # Y = 0: the curve has no such point; the double is the identity all the same
    ask("jdbl", list(G[0]) + list(G[1]) + [0, 0], [0, 0, 0, 0, 1])                                  # Z = 0
    z = red(rnd2())
    z2 = model.f2_sqr(z)
    ask("jdbl", list(model.f2_mul(G[0], z2)) + list(model.f2_mul(G[1], model.f2_mul(z2, z))) + list(z), pt5(model.add(G, G)))
    ks = [0, 1, 2, 15, 16, R - 1, R, R + 1, 2**256 - 1, 2**255] + [rng.getrandbits(256) for _ in range(3)]
    for k in ks:
        for pt in (G, off[1]):
            ask("pmul", [k] + pt5(pt)[:4], pt5(model.mul(k, pt)))                                   # integer semantics: off[1] is not in G2
    for r in model.point_records(fx)[1:]:
        ask("subgroup", pt5(dec(r))[:4], [1 if r["in_subgroup"] else 0])
    w48 = lambda b: [int.from_bytes(b[j:j + 48], "big") for j in range(0, len(b), 48)]
    cls_of = lambda pt: [2, 0, 0, 0, 0] if pt is model.MALFORMED else [0, 0, 0, 0, 0] if pt is INF else [1] + pt5(pt)[:4]
    for r in model.point_records(fx):
        u, c = bytes.fromhex(r["uncompressed"]), bytes.fromhex(r["compressed"])
        pt = dec(r)
        ask("dec192", w48(u), cls_of(pt)); ask("dec96", w48(c), cls_of(pt))
        ask("enc", pt5(pt)[4:] + pt5(pt)[:4], w48(u) + w48(c))
    for m in fx["malformed_uncompressed"]:
        ask("dec192", w48(bytes.fromhex(m["bytes"])), [2, 0, 0, 0, 0])
    for m in fx["malformed_compressed"]:
        ask("dec96", w48(bytes.fromhex(m["bytes"])), [2, 0, 0, 0, 0])
    out = subprocess.run([str(exe)], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=900)
    lines = out.stdout.strip().split("\n")
    assert out.returncode == 0 and len(lines) == len(reqs), out.stderr[-500:]
    wrong = []
    for r, e, chk, l in zip(reqs, exps, checks, lines):
        got = [int(x, 16) for x in l.split()]
        if (e is not None and got != [v % (1 << 384) for v in e]) or (chk is not None and not chk(got)):
            wrong.append((r[:120], l[:300]))
    assert not wrong, (len(wrong), wrong[:5])


# ---- the C ABI and the plans
def test_the_functions_are_declared_in_their_own_header_and_exported(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols, declared_bls12_381_symbols, declared_bls12_381_g2_symbols
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(ecsimd_bls381_g2_[a-z0-9_]+)\s*\(", text))
    assert declared == SYMBOLS == set(declared_bls12_381_g2_symbols())
    assert not re.search(r"\becsimd_bls12_381_[a-z0-9_]+\s*\(", text.split("#ifndef")[1])        # no name under the G1 prefix is declared here
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert {s for s in exported if s.startswith("ecsimd_bls381_g2")} == declared
    assert {s for s in exported if s.startswith("ecsimd_bls12_381")} == G1_SYMBOLS == set(declared_bls12_381_symbols())   # unchanged
    assert {s for s in exported if s.startswith("ecsimd_hip_")} == set(declared_symbols())                                # unchanged
    assert "PUBLIC DATA ONLY" in text and "h2" in text and "NOT IN G2" in text and '#include "ecsimd_msm.h"' in text
    from ecsimd_amd import Engine
    for m in ("decompress", "compress", "check", "mul", "msm", "point_sum", "msm_plan", "raw"):
        assert callable(getattr(Engine, "bls12_381_g2_" + m)), m
    ins, outs = (4, 2, 4, 4, 2, 2, 2, 2, 10, 5, 9), (2, 2, 2, 2, 2, 2, 3, 2, 5, 5, 5)
    assert tuple(built.ecsimd_bls381_g2_raw_inputs(op) for op in range(11)) == ins and tuple(built.ecsimd_bls381_g2_raw_outputs(op) for op in range(11)) == outs
    for fn in (built.ecsimd_bls381_g2_raw_inputs, built.ecsimd_bls381_g2_raw_outputs):
        assert fn(-1) == 0 and fn(11) == 0


def plan_of(lib, name, n, bits, flags):
    from ecsimd_amd.engine import MsmPlan
    p = MsmPlan()
    rc = getattr(lib, name)(C.c_size_t(n), C.c_int(bits), C.c_int(flags), C.byref(p))
    return None if rc != 0 else {f: int(getattr(p, f)) for f in FIELDS}


def threshold():
    m = re.search(r"#define ECSIMD_BLS381_G2_MSM_AUTO_THRESHOLD \(\(size_t\)1 << (\d+)\)", open(HEADER).read())
    return 1 << int(m.group(1))


def test_g2_msm_plan_is_the_models_restatement_of_the_schedule(built):
    built.ecsimd_bls381_g2_msm_plan.restype = C.c_int
    th = threshold()
    for n in NS + (th - 1, th, 2**24):
        for bits in BITS:
            for flags in (0, 1, 2):
                got = plan_of(built, "ecsimd_bls381_g2_msm_plan", n, bits, flags)
                assert got == model.plan(n, bits, flags, th), (n, bits, flags)
                if flags == 2 and n:
                    assert got["workspace_bytes"] == 16 + 288 * n and got["launches"] == 3 + g1_model._tree_passes(n)
            a, b = plan_of(built, "ecsimd_bls381_g2_msm_plan", n, bits, 1), plan_of(built, "ecsimd_bls12_381_g1_msm_plan", n, bits, 1)
            assert {f: a[f] for f in FIELDS[:-1]} == {f: b[f] for f in FIELDS[:-1]}                # one schedule, wider elements
            assert a["workspace_bytes"] > b["workspace_bytes"] or n == 0
    for n, bits, flags in ((1, 0, 0), (1, 257, 0), (2**24 + 1, 255, 0), (1, 255, 3), (1, 255, -1)):
        assert plan_of(built, "ecsimd_bls381_g2_msm_plan", n, bits, flags) is None and model.plan(n, bits, flags, th) is None
    assert built.ecsimd_bls381_g2_msm_plan(C.c_size_t(1), C.c_int(255), C.c_int(0), None) != 0


def test_the_shipped_listing_has_the_figures_the_profile_records(built):
    """tools/bls12_381_listing.py --unit g2 --check on the listing the build left in build/csrc, and, said per figure, what no change of the unit may move
    unnoticed: every kernel's and out-of-line function's instruction counts, registers, scratch and spills.  Kernel names, resource lines and instruction counts only."""
    import bls12_381_listing as listing
    path = os.path.join(ROOT, "build", "csrc", listing.UNITS["g2"]["listing"] + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(path), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    for f in ("k_bls12_381_g2.hip", "k_bls12_381.inc", "bls381_curve.inc", "g2.cuh", "fp2.cuh", "fe381.cuh", "fe384.cuh", "bls381_bytes.cuh", "msm_stages.cuh", "kernels.h"):
        assert os.path.getmtime(path) >= os.path.getmtime(os.path.join(CSRC, f)), f
    got, recorded = listing.report("g2"), json.load(open(os.path.join(ROOT, listing.UNITS["g2"]["out"])))
    assert len(recorded["kernels"]) == 14 and sorted(recorded["functions"]) == ["g2_add", "g2_dbl", "g2_madd"]
    for section in ("kernels", "functions"):
        for name, figures in recorded.get(section, {}).items():
            for f in ("valu", "mads", "registers", "agprs", "vgprs", "private_segment_fixed_size", "scratch_bytes", "vgpr_spill_count", "text_bytes"):
                if f in figures:
                    assert got[section][name][f] == figures[f], (name, f, got[section][name][f], figures[f])
    assert got == recorded, f"{listing.UNITS['g2']['out']} is stale: python tools/bls12_381_listing.py --unit g2"
