#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of k_p384.hip (build/csrc/k_p384-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r18/p384_listing.json: per kernel the VALU and multiply (v_mad_u64_u32) counts of its text, the VGPR allocation (architectural + accumulation
registers: one 512-entry file per lane on gfx950) with the waves per SIMD it allows, and scratch; for one complete addition the counts of its loop body; and the
a-priori figure they imply -- VALU instructions per verification, beside the same figure for P-256's ecdsa_verify loop where its listing is there -- to hold
the measured rate of tools/time_p384.py against.

    python tools/p384_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                                   # noqa: E402
from ed25519_listing import counts, longest_loop  # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_p384-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r18", "p384_listing.json")
KERNELS = ("k_p384_sha384", "k_p384_pubkey", "k_p384_ecdh", "k_p384_sign_nonce", "k_p384_sign_finish", "k_p384_verify", "k_p384_raw")
MUL_MADS, SQR_MADS = 144, 78


def waves_per_simd(registers):
    """gfx950: 512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves."""
    return max(1, min(8, 512 // ((registers + 7) // 8 * 8)))


def report():
    asm = open(LISTING).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_p384.hip (tools/p384_listing.py).  Per kernel: VALU instructions and v_mad_u64_u32 in its TEXT (loops "
                      "counted once), registers = the allocation out of the 512 per lane (VGPRs and AGPRs are one file), the waves per SIMD that allows, "
                      "scratch bytes.  A field product is 144 v_mad_u64_u32, a squaring 78; the reduction multiplies nothing.  add_loop_body: the text of "
                      "the longest loop with a short backward branch in k_p384_verify / k_p384_ecdh -- the table's complete additions, ONE Algorithm 4: 14 "
                      "products (2016 v_mad_u64_u32) with their reductions, additions and moves (the window loops are too long for a short branch and are "
                      "not measured this way).  *_mads_per_lane: 96 windows x (4 doublings of 3 squarings + 8 products, a mixed addition of 13 products and, "
                      "in verification, a complete one of 14) + the table's 7 additions (+ ECDH's inversion).  verify_valu_per_lane: verify_mads_per_lane x "
                      "the VALU per v_mad_u64_u32 of add_loop_body; a-priori, not a measurement.",
           "kernels": {}}
    for name in KERNELS:
        insts = [i for _, _, x in ct_check.parse_function(asm, name) for i in x]
        b = [v for k, v in blocks.items() if name in k][0]
        regs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        out["kernels"][name] = dict(counts(insts), registers=regs, agprs=int(b.split()[0]), waves_per_simd=waves_per_simd(regs),
                                    private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    out["add_loop_body"] = counts(longest_loop(asm, "k_p384_verify"))
    out["ecdh_add_loop_body"] = counts(longest_loop(asm, "k_p384_ecdh"))
    # field work per verification: 96 windows x (4 doublings of 3 squarings + 8 products, a mixed addition of 11 products + 2 by b counted in, a complete one of 12 + 2)
    dbl = 3 * SQR_MADS + 8 * MUL_MADS
    out["verify_mads_per_lane"] = 96 * (4 * dbl + 13 * MUL_MADS + 14 * MUL_MADS) + 7 * 14 * MUL_MADS
    out["ecdh_mads_per_lane"] = 96 * (4 * dbl + 14 * MUL_MADS) + 7 * 14 * MUL_MADS + 383 * SQR_MADS + 15 * MUL_MADS
    out["verify_valu_per_lane"] = round(out["verify_mads_per_lane"] * out["add_loop_body"]["valu"] / out["add_loop_body"]["mads"])
    out["p256_comparison"] = {"naive_work_ratio": round((12 / 8) ** 2 * 384 / 256, 2),
                              "note": "P-256's ecdsa_verify multiplies 8 x 8 words (64 v_mad_u64_u32 a product) over 256 bits"}
    return out


def dump(r):
    """One kernel per line."""
    line = lambda v: json.dumps(v, separators=(", ", ": "))
    body = ",\n".join(' %s: {\n%s\n }' % (json.dumps(k), ",\n".join('  %s: %s' % (json.dumps(n), line(c)) for n, c in v.items())) if k == "kernels" else ' %s: %s' % (json.dumps(k), line(v))
                      for k, v in r.items())
    return "{\n" + body + "\n}\n"


if __name__ == "__main__":
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r18/p384_listing.json is stale: python tools/p384_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(dump(r))
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
