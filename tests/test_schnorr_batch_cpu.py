"""BIP-340 batch verification without a GPU (include/ecsimd_schnorr_batch.h): the host model of the method against signature-by-signature verification, the
tag midstates the device source holds as literals, the host-only plan, and the C boundary."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bip340_model as b340            # noqa: E402
import schnorr_batch_model as model    # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ecsimd_schnorr_batch.h")
NAMES = ("ecsimd_schnorr_batch_plan", "ecsimd_schnorr_verify_batch", "ecsimd_schnorr_batch_randomizers")
AUTO, MSM, LANES = 0, 1, 2
MAX_N = (1 << 24) - 1
BAD_ARG = -1


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


def batch(u, msg_bytes=32):
    """u valid signatures: keys 1, n - 1 and a few between, messages of one length."""
    keys = [1, b340.N - 1] + [0xB7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFEF * (i + 1) % b340.N for i in range(u)]
    msgs = [bytes((7 * i + j) & 0xff for j in range(msg_bytes)) for i in range(u)]
    sigs = [b340.sign(keys[i], msgs[i], i) for i in range(u)]
    return [s[0] for s in sigs], msgs, [s[1] for s in sigs], [s[2] for s in sigs]


def lane_by_lane(pxs, msgs, rs, ss):
    return all(b340.verify(px, m, r, s) for px, m, r, s in zip(pxs, msgs, rs, ss))


# ---- the model
def test_the_model_accepts_what_verify_accepts_one_by_one():
    assert model.batch_verify([], [], [], [])
    for u, length in ((1, 32), (2, 0), (5, 33), (8, 32)):
        pxs, msgs, rs, ss = batch(u, length)
        assert lane_by_lane(pxs, msgs, rs, ss) and model.batch_verify(pxs, msgs, rs, ss)
        a = model.randomizers(pxs, msgs, rs, ss)
        assert len(a) == u and all(x & 1 and x < 1 << 128 for x in a)


def test_the_model_refuses_forged_and_malformed_lanes():
    pxs, msgs, rs, ss = batch(6)
    for lane in (0, 3, 5):
        for what in ("s", "r", "px", "msg", "s=n", "r>=p", "px>=p", "r off", "px off"):
            p2, m2, r2, s2 = list(pxs), list(msgs), list(rs), list(ss)
            if what == "s": s2[lane] ^= 1 << 9
            elif what == "r": r2[lane] = rs[(lane + 1) % 6]
            elif what == "px": p2[lane] = pxs[(lane + 2) % 6]     # (+ 2: keys 1 and n - 1, lanes 0 and 1, share their x-only key)
            elif what == "msg": m2[lane] = bytes([msgs[lane][0] ^ 4]) + msgs[lane][1:]
            elif what == "s=n": s2[lane] = b340.N
            elif what == "r>=p": r2[lane] = b340.P + 1          # x = 1 is on the curve: refused for its range alone
            elif what == "px>=p": p2[lane] = b340.P + 1
            elif what == "r off": r2[lane] = 5                   # 5^3 + 7 is no square
            elif what == "px off": p2[lane] = 5
            assert not lane_by_lane(p2, m2, r2, s2), (lane, what)
            assert not model.batch_verify(p2, m2, r2, s2), (lane, what)
    assert b340.lift_x(1) is not None and b340.lift_x(5) is None


def test_errors_that_cancel_in_the_unweighted_sum_are_refused_by_the_weights():
    """s_i + d and s_j - d leave sum s_i unchanged: with every a_i = 1 the batch equation still holds, with the model's randomizers it does not.  The same with
    lanes i and j exact copies of one signature, where only the lane index tells the two a_i apart."""
    pxs, msgs, rs, ss = batch(6)
    delta = 0x1234567
    s2 = list(ss); s2[1] = (ss[1] + delta) % b340.N; s2[4] = (ss[4] - delta) % b340.N
    assert not lane_by_lane(pxs, msgs, rs, s2)
    assert model.batch_verify(pxs, msgs, rs, s2, a=[1] * 6) and not model.batch_verify(pxs, msgs, rs, s2)
    px, m, r, s = pxs[2], msgs[2], rs[2], ss[2]
    twins = ([px] * 2, [m] * 2, [r] * 2, [(s + delta) % b340.N, (s - delta) % b340.N])
    assert model.batch_verify(*twins, a=[1, 1]) and not model.batch_verify(*twins)
    a = model.randomizers(*twins)
    assert a[0] != a[1]
    assert model.batch_verify([px] * 2, [m] * 2, [r] * 2, [s] * 2)


def test_every_randomizer_depends_on_every_lane_and_on_the_batch_length():
    pxs, msgs, rs, ss = batch(5)
    a = model.randomizers(pxs, msgs, rs, ss)
    s2 = list(ss); s2[3] ^= 1
    assert all(x != y for x, y in zip(a, model.randomizers(pxs, msgs, rs, s2)))
    m2 = list(msgs); m2[0] = bytes([msgs[0][0] ^ 1]) + msgs[0][1:]
    assert all(x != y for x, y in zip(a, model.randomizers(pxs, m2, rs, ss)))
    assert all(x != y for x, y in zip(a, model.randomizers(pxs[:4], msgs[:4], rs[:4], ss[:4])))
    # the tree: 17 leaves are two levels, and the root of one leaf is the leaf
    leaves = [bytes([i]) * 32 for i in range(17)]
    level1 = [b340.tagged_hash(model.TAG_NODE, b"".join(leaves[:16])), b340.tagged_hash(model.TAG_NODE, leaves[16])]
    assert model.root(leaves) == b340.tagged_hash(model.TAG_NODE, level1[0] + level1[1]) and model.root(leaves[:1]) == leaves[0]


# ---- the device source
def test_the_midstates_in_the_device_source_are_hashlibs():
    src = open(os.path.join(CSRC, "k_schnorr_batch.hip")).read()
    table = re.search(r"SCHNORR_BATCH_MID\[5\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [[int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", row)] for row in re.findall(r"\{([^{}]*)\}", table)]
    assert len(rows) == 5 and all(len(r) == 8 for r in rows)
    order = re.search(r'tag = "([\w/-]+)", "([\w/-]+)", "([\w/-]+)",\s*//\s*"([\w/-]+)", "([\w/-]+)"', src).groups()
    assert order == model.DEVICE_TAGS == (model.TAG_LEAF, model.TAG_NODE, model.TAG_SEED, model.TAG_A, "BIP0340/challenge")
    for tag, row in zip(model.DEVICE_TAGS, rows):
        assert row == b340.midstate(tag), tag
        for length in (0, 40, 64, 96, 512):
            data = bytes(range(256)) * 2
            assert b340.finish_from_midstate(row, data[:length]) == b340.tagged_hash(tag, data[:length])


# ---- the plan
def plan(lib, n, msg_bytes=32, flags=AUTO):
    from ecsimd_amd.engine import SchnorrBatchPlan
    p = SchnorrBatchPlan()
    rc = lib.ecsimd_schnorr_batch_plan(C.c_size_t(n), C.c_size_t(msg_bytes), C.c_int(flags), C.byref(p))
    return rc, p


def threshold():
    m = re.search(r"#define ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD\s+(.*)", open(HEADER).read()).group(1).strip()
    if "SIZE_MAX" in m:
        return None
    return 1 << int(re.fullmatch(r"\(\(size_t\)1 << (\d+)\)", m).group(1))


def tree_passes(c):
    p = 0
    while c > 1:
        c = (c + 15) // 16; p += 1
    return p


def test_the_plan_routes_counts_and_sizes(built):
    from ecsimd_amd import Engine
    t = threshold()
    if t is None:
        assert plan(built, MAX_N)[1].route == LANES
    else:
        assert t <= MAX_N and plan(built, t - 1)[1].route == LANES and plan(built, t)[1].route == MSM and plan(built, MAX_N)[1].route == MSM
    assert plan(built, 5, flags=MSM)[1].route == MSM and plan(built, MAX_N, flags=LANES)[1].route == LANES
    for flags in (AUTO, MSM, LANES):
        rc, p = plan(built, 0, flags=flags)
        assert rc == 0 and p.launches == 1 and p.workspace_bytes == 0
    # the launch counts the header states
    for n in (1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097, 65537, 1 << 20, (1 << 22) + 1, MAX_N):
        rc, p = plan(built, n, flags=MSM)
        levels = tree_passes(n)
        want = 5 + levels + max(1, levels) + Engine.msm_plan(n, 128, 1)["launches"] + Engine.msm_plan(n + 1, 256, 1)["launches"]
        assert rc == 0 and p.launches == want, (n, p.launches, want)
        rc, p = plan(built, n, flags=LANES)
        assert rc == 0 and p.launches == 1 + 9 * ((n + (1 << 22) - 1) >> 22), n
        assert Engine.schnorr_batch_plan(n, 32, MSM) == dict(route=MSM, launches=want, workspace_bytes=plan(built, n, flags=MSM)[1].workspace_bytes)
    # the workspace never shrinks as n grows -- the bucket sums' own need does, next to every power of two -- and holds both sums and the call's arrays
    for flags in (MSM, LANES):
        last = 0
        sizes = sorted(set(range(1, 2200)) | {v for k in range(11, 25) for v in ((1 << k) - 2, (1 << k) - 1, 1 << k, (1 << k) + 1, 3 << (k - 1)) if v <= MAX_N})
        for n in sizes:
            w = plan(built, n, flags=flags)[1].workspace_bytes
            assert w >= last, (flags, n, w, last)
            last = w
            if flags == MSM:
                assert w >= 288 * n + max(Engine.msm_plan(n, 128, 1)["workspace_bytes"], Engine.msm_plan(n + 1, 256, 1)["workspace_bytes"])
    assert Engine.msm_plan(255, 256, 1)["workspace_bytes"] > Engine.msm_plan(256, 256, 1)["workspace_bytes"]      # what the plan has to smooth over
    # the message length does not enter the sizes
    assert [plan(built, 1000, m, MSM)[1].workspace_bytes for m in (0, 33, 1 << 20)] == [plan(built, 1000, 32, MSM)[1].workspace_bytes] * 3


def test_the_plan_refuses_what_the_call_refuses(built):
    from ecsimd_amd import Engine, EcsimdHipError
    assert plan(built, MAX_N)[0] == 0 and plan(built, MAX_N + 1)[0] == BAD_ARG
    assert plan(built, 8, flags=3)[0] == BAD_ARG and plan(built, 8, flags=4)[0] == BAD_ARG and plan(built, 8, flags=-1)[0] == BAD_ARG
    assert plan(built, 8, msg_bytes=(1 << 40) + 1)[0] == BAD_ARG and plan(built, 8, msg_bytes=1 << 40)[0] == 0
    assert built.ecsimd_schnorr_batch_plan(C.c_size_t(8), C.c_size_t(32), C.c_int(0), None) == BAD_ARG
    with pytest.raises(EcsimdHipError):
        Engine.schnorr_batch_plan(MAX_N + 1, 32)
    # no context: the two calls refuse before they touch anything
    assert built.ecsimd_schnorr_verify_batch(None, None, None, C.c_size_t(0), C.c_size_t(0), None, None, None, C.c_size_t(0), C.c_int(0)) == BAD_ARG
    assert built.ecsimd_schnorr_batch_randomizers(None, None, None, C.c_size_t(0), C.c_size_t(0), None, None, None, C.c_size_t(0)) == BAD_ARG


# ---- the boundary
def test_the_header_is_c99_and_a_caller_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_schnorr_batch.h"
#include <stddef.h>
int main(int argc, char** argv) {
  ecsimd_schnorr_batch_plan_t p;
  uint64_t* w = NULL; uint8_t* b = NULL; (void)argv;
  if (ecsimd_schnorr_batch_plan(17, 32, ECSIMD_SCHNORR_BATCH_MSM, &p) != ECSIMD_HIP_OK || p.route != ECSIMD_SCHNORR_BATCH_MSM || p.launches < 10) return 1;
  if (ecsimd_schnorr_batch_plan(ECSIMD_MSM_MAX_N, 32, ECSIMD_SCHNORR_BATCH_AUTO, &p) != ECSIMD_HIP_ERR_BAD_ARG) return 2;
  if (ECSIMD_SCHNORR_BATCH_AUTO_THRESHOLD < 2) return 3;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_schnorr_verify_batch(NULL, w, b, 32, 32, w, w, b, 0, ECSIMD_SCHNORR_BATCH_LANES);
    rc |= ecsimd_schnorr_batch_randomizers(NULL, w, b, 32, 40, w, w, w, 0);
    return rc;
  }
  return 0;
}
''')
    libdir = os.path.join(ROOT, "ecsimd_amd")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lecsimd_hip", "-Wl,-rpath," + libdir], check=True)
    assert subprocess.run([str(exe)]).returncode == 0          # the plan is host only: it runs here


def test_the_three_names_are_exported_and_the_other_header_is_as_it_was(built):
    import ecsimd_amd
    from ecsimd_amd.engine import declared_symbols
    out = subprocess.run(["nm", "-D", "--defined-only", ecsimd_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)$", out, re.M))
    for name in NAMES:
        assert name in exported and hasattr(built, name), name
    assert not [s for s in declared_symbols() if "batch" in s]
    assert sorted(s for s in exported if s.startswith("ecsimd_hip_")) == declared_symbols()
    assert re.findall(r"\b(ecsimd_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)) == list(NAMES)
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_schnorr_batch.hip" in text and "ecsimd_schnorr_batch.h" in text
    from ecsimd_amd import Engine, flags
    assert (flags.SCHNORR_BATCH_AUTO, flags.SCHNORR_BATCH_MSM, flags.SCHNORR_BATCH_LANES) == (AUTO, MSM, LANES)
    for m in ("schnorr_verify_batch", "schnorr_batch_randomizers", "schnorr_batch_plan"):
        assert callable(getattr(Engine, m))
