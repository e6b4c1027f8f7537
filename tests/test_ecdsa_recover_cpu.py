"""ECDSA public-key recovery and recoverable signing, the part that needs no GPU: the two entry points are declared, exported and callable from C99;
the new kernels exist in the shipped gfx950 listing without scratch memory; the kernel that forms the recovery id keeps the affine k G and s out of every
branch condition and address (tools/ct_check.py check_secret_flow), and the analysis refuses a planted branch on the parity of y; and the host model the GPU
tests take their expected values from (tools/ecdsa_recover_model.py) agrees with the textbook ec_mul of tests/helpers.py."""
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                      # noqa: E402
import ecdsa_recover_model as model  # noqa: E402
from helpers import CURVE_PARAMS, P256, SECP256K1, ec_add, ec_mul  # noqa: E402

CSRC = os.path.join(ROOT, "ecsimd_amd", "csrc")
NEW_SYMBOLS = ("ecsimd_hip_ecdsa_recover", "ecsimd_hip_ecdsa_sign_recoverable")
NEW_KERNELS = ("14k_recover_liftILi0EE", "14k_recover_liftILi1EE", "17k_gc_recover_lift", "23k_ecdsa_recover_scalars", "18k_sign_recovery_id")


def curve_dicts():
    from ecsimd_amd.curves import NAMED
    return {"p256": CURVE_PARAMS[P256], "secp256k1": CURVE_PARAMS[SECP256K1], **NAMED}


@pytest.fixture(scope="module")
def built():
    import ecsimd_amd
    subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", CSRC, "ARCH=gfx950"], check=True, capture_output=True, timeout=1800)
    return ecsimd_amd.load_library()


@pytest.fixture(scope="module")
def recover_asm(built):
    listing = os.path.join(ROOT, "build", "csrc", "k_recover-hip-amdgcn-amd-amdhsa-gfx950.s")
    assert os.path.exists(listing), "the Makefile no longer leaves the device listings in build/csrc (-save-temps=obj)"
    assert os.path.getmtime(listing) >= os.path.getmtime(os.path.join(CSRC, "k_recover.hip")), listing
    return open(listing).read()


# ---- 7. the C ABI
def test_both_entry_points_are_declared_and_exported(built):
    from ecsimd_amd.engine import declared_symbols
    from ecsimd_amd import ECDSA_LOW_S
    syms = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(built, s), s
    header = open(os.path.join(ROOT, "include", "ecsimd_hip.h")).read()
    assert re.search(r"ECSIMD_HIP_ECDSA_LOW_S\s*=\s*%d\b" % ECDSA_LOW_S, header)


def test_a_c99_caller_compiles_and_links(built, tmp_path):
    src = tmp_path / "caller.c"
    src.write_text('''#include "ecsimd_hip.h"
#include <stddef.h>
int main(int argc, char** argv) {
  uint64_t* w = NULL; uint8_t* b = NULL; (void)argv;
  if (argc > 1000) {   /* never taken: the calls only have to compile against the prototypes and resolve at link time */
    int rc = ecsimd_hip_ecdsa_recover(NULL, ECSIMD_HIP_SECP256K1, w, w, w, b, w, NULL, b, 0);
    rc |= ecsimd_hip_ecdsa_sign_recoverable(NULL, ECSIMD_HIP_P256, w, w, w, w, w, b, b, 0, ECSIMD_HIP_ECDSA_LOW_S);
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


# ---- 8. the shipped ISA
def test_new_kernels_exist_and_use_no_scratch(recover_asm):
    meta = recover_asm[recover_asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    for k in NEW_KERNELS:
        hit = [b for name, b in blocks.items() if k in name]
        assert len(hit) == 1, k
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", hit[0]), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", hit[0]) and re.search(r"\.sgpr_spill_count:\s+0\b", hit[0]), k
    assert "scratch_" not in recover_asm
    assert "k_recover.hip" in open(os.path.join(CSRC, "Makefile")).read()


# arguments of k_sign_recovery_id: (order, x, y, s, ok, v, n, low_s) -- order is 32 bytes BY VALUE: one argument.  Secret: the affine k G and the s that comes in.
ID_KERNEL, ID_SECRETS = "k_sign_recovery_id", [1, 2, 3]


def test_recovery_id_kernel_keeps_the_point_and_s_out_of_control_flow_and_addresses(recover_asm):
    rep = ct_check.check_secret_flow(recover_asm, ID_KERNEL, secret_args=ID_SECRETS)
    assert rep["secret_loads"] >= 3 and not rep["secret_scratch"] and not rep["secret_lds"]
    assert rep["public_branches"] >= 1            # the batch's tail, on the public element index
    for a, name in ((1, "x"), (2, "y"), (3, "s")):
        assert ct_check.check_secret_flow(recover_asm, ID_KERNEL, secret_args=[a])["secret_loads"] >= 1, name
    # the front end of recovery handles public data and says so: its validity checks ARE branches on loaded values
    with pytest.raises(ct_check.Violation):
        ct_check.check_secret_flow(recover_asm, "k_ecdsa_recover_scalars", secret_args=[2])


def test_the_analysis_refuses_a_branch_on_the_parity_of_y(recover_asm):
    """The mutation: right after the load of y's low word, `if (y & 1) goto ...`.  With y secret the analysis has to refuse it; the control, the same
    branch fed from the work-item id, passes."""
    lines = recover_asm.splitlines()
    fn = next(i for i, ln in enumerate(lines) if re.match(r"^_ZN\w*%s\w*:" % ID_KERNEL, ln))
    end = next(i for i in range(fn, len(lines)) if lines[i].startswith(".Lfunc_end"))
    label = next(b[0] for b in ct_check.parse_function(recover_asm, ID_KERNEL) if b[0].startswith(".LBB"))
    plant = lambda reg: ["\ts_waitcnt vmcnt(0)", f"\tv_and_b32_e32 v250, 1, {reg}", "\tv_cmp_ne_u32_e32 vcc, 0, v250", f"\ts_cbranch_vccnz {label}"]
    refused = 0
    for i in range(fn, end):
        m = re.match(r"\s*global_load_\w+ v\[?(\d+)", lines[i])
        if not m:
            continue
        mutated = "\n".join(lines[:i + 1] + plant(f"v{m.group(1)}") + lines[i + 1:])
        try:
            ct_check.check_secret_flow(mutated, ID_KERNEL, secret_args=[2])       # y alone is secret here: only ITS loads may trip the analysis
        except ct_check.Violation as exc:
            assert "VCC" in str(exc) or "condition" in str(exc), exc
            refused += 1
            ct_check.check_secret_flow(mutated, ID_KERNEL, secret_args=[1])     # only x secret: the same text passes, the branch is on y
    assert refused >= 1, "no load of y that the analysis treats as secret"
    ct_check.check_secret_flow("\n".join(lines[:fn + 1] + plant("v0") + lines[fn + 1:]), ID_KERNEL, secret_args=ID_SECRETS)


# ---- 9. the host model against the textbook ec_mul
@pytest.mark.parametrize("cv", [P256, SECP256K1])
def test_host_model_against_textbook_ec_mul(cv):
    c = CURVE_PARAMS[cv]
    G = (c["gx"], c["gy"])
    rng = random.Random(600 + cv)
    seen = set()
    for i in range(64):
        e, d, k = rng.getrandbits(256), rng.randrange(1, c["n"]), rng.randrange(1, c["n"])
        kG, Q = ec_mul(cv, k, G), ec_mul(cv, d, G)
        low = bool(i & 1)
        r, s, v = model.sign_recoverable(c, e, d, k, low_s=low, kG=kG)
        rr = kG[0] % c["n"]
        ss = pow(k, -1, c["n"]) * (e + rr * d) % c["n"]
        flipped = low and ss > c["n"] // 2
        assert (r, s) == (rr, c["n"] - ss if flipped else ss) and v == ((kG[1] & 1) ^ flipped) | (2 if kG[0] >= c["n"] else 0)
        assert not low or s <= c["n"] // 2
        seen.add(v)
        assert model.recover(c, e, r, s, v) == Q, i
        assert model.recover(c, e % c["n"], r, s, v) == Q                                          # e is reduced mod n
        other = model.recover(c, e, r, s, v ^ 1)                                                   # the other root: r^-1 (-s R - e G), a different key
        u = pow(r, -1, c["n"])
        minus_R = (kG[0], c["p"] - kG[1]) if not flipped else kG
        want = ec_mul(cv, u * s % c["n"], minus_R)
        eg = ec_mul(cv, (c["n"] - e * u) % c["n"], G)
        assert other == ec_add(cv, eg, want) and other != Q
        # the front end by itself: the scalars and the point
        valid, u1, u2, R = model.front_end(c, e, r, s, v)
        assert valid and u1 == (-e * u) % c["n"] and u2 == s * u % c["n"] and R[0] == kG[0] and (R[1] * R[1] - R[0] ** 3 - c["a"] * R[0] - c["b"]) % c["p"] == 0
        for bad in ((0, s, v), (r, 0, v), (c["n"], s, v), (r, c["n"], v), (2**256 - 1, s, v), (r, s, 4), (r, s, 255)):
            assert model.recover(c, e, *bad) is None and model.front_end(c, e, *bad) == (False, 0, 0, G)
    assert seen >= {0, 1}
    # Q at infinity: R = k G, e = s k mod n  ->  -e/r G + s/r R = 0
    k, s = rng.randrange(1, c["n"]), rng.randrange(1, c["n"])
    kG = ec_mul(cv, k, G)
    assert model.front_end(c, s * k % c["n"], kG[0] % c["n"], s, kG[1] & 1)[0] and model.recover(c, s * k % c["n"], kG[0] % c["n"], s, kG[1] & 1) is None


def test_second_x_candidate_values_of_the_issue():
    """r + n below p and on the curve: r = 3, 4, 6, 9 on P-256 and r = 2, 4, 6, 7 on secp256k1 (what tests/test_gpu_ecdsa_recover.py builds test 3 from)."""
    for cv, rs in ((P256, (3, 4, 6, 9)), (SECP256K1, (2, 4, 6, 7))):
        c = CURVE_PARAMS[cv]
        for r in rs:
            assert r + c["n"] < c["p"] and model.is_square(c, r + c["n"])
            R = model.lift(c, r, 2)
            assert R is not None and R[0] == r + c["n"] and R[1] % 2 == 0 and ec_mul(cv, c["n"], R) is None
            assert model.lift(c, r, 3) == (R[0], c["p"] - R[1])
        assert model.lift(c, c["p"] - c["n"], 2) is None and model.lift(c, c["p"] - c["n"] + 5, 3) is None       # x = r + n >= p


@pytest.mark.parametrize("name", ["brainpoolP256r1", "sm2", "frp256v1"])
def test_host_model_round_trips_on_the_named_curves(name):
    c = curve_dicts()[name]
    assert c["p"] % 4 == 3
    G = (c["gx"], c["gy"])
    rng = random.Random(name)
    for i in range(64):
        e, d, k = rng.getrandbits(256), rng.randrange(1, c["n"]), rng.randrange(1, c["n"])
        r, s, v = model.sign_recoverable(c, e, d, k, low_s=bool(i & 1))
        assert model.recover(c, e, r, s, v) == model.ec_mul(c, d, G)


@pytest.mark.parametrize("cv", [P256, SECP256K1])
def test_the_models_lift_agrees_with_eulers_criterion(cv):
    c = CURVE_PARAMS[cv]
    rng = random.Random(900 + cv)
    xs = [rng.randrange(1, c["n"]) for _ in range(256)]
    verdicts = [model.lift(c, x, 0) is not None for x in xs]
    assert verdicts == [model.is_square(c, x) for x in xs] and 64 < sum(verdicts) < 192
    for x in xs[:32]:
        R0, R1 = model.lift(c, x, 0), model.lift(c, x, 1)
        assert (R0 is None) == (R1 is None) and (R0 is None or (R0[0] == R1[0] == x and R0[1] + R1[1] == c["p"] and R0[1] % 2 == 0))
