#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of k_x25519.hip (build/csrc/k_x25519-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r14/x25519_listing.json: per kernel the VALU and multiply (v_mad_u64_u32) counts, the registers, scratch and LDS; the counts of one ladder step (the
body of k_x25519's longest loop) and of one comb row (k_x25519_base's); and the a-priori VALU instructions per call they imply, to hold the measured rates of
tools/time_x25519.py against.

    python tools/x25519_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                                     # noqa: E402
from ed25519_listing import counts, longest_loop    # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_x25519-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r14", "x25519_listing.json")
KERNELS = {"k_x25519": "8k_x25519E", "k_x25519_base": "13k_x25519_base", "k_x25519_from_ed_pk": "19k_x25519_from_ed_pk", "k_x25519_from_ed_seed": "21k_x25519_from_ed_seed",
           "k_x25519_raw": "12k_x25519_raw"}
MUL_MADS, SQR_MADS, SMALL_MADS = 72, 44, 8          # fe25519_mul: 64 column products + 8 of the fold by 38; fe25519_sqr: 28 + 8 + 8; fe25519_mul_small: 8
INVERT_SQR, INVERT_MUL = 254, 11                    # fe25519_invert


def report():
    asm = open(LISTING).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_x25519.hip (tools/x25519_listing.py).  Per kernel: VALU instructions and v_mad_u64_u32 in its text, VGPRs, "
                      "scratch and LDS bytes.  ladder_step: the body of k_x25519's longest loop, one step of RFC 7748's ladder (5 products, 4 squarings, one "
                      "product by 121665, 8 additions, two masked swaps); comb_row: the body of k_x25519_base's longest loop, one row of the comb (a selection "
                      "over eight entries and a mixed addition).  ladder_step_mads_expected: 5 x 72 + 4 x 44 + 8, and the two multiply-adds by 38 of fe25519_fold_carry behind each "
                      "of the 10 products and 4 additions.  inversion_valu: 254 squarings and 11 "
                      "products at the step's VALU per v_mad_u64_u32 (an estimate: the chain's loops are a few squarings each in the text).  "
                      "x25519_valu_per_lane: 255 steps + the rest of the kernel's text once + the inversion; x25519_base_valu_per_lane: 64 rows + the rest of "
                      "the text once + the inversion.  A-priori figures, not measurements: profiles/r14/x25519.txt is tools/time_x25519.py's to write.",
           "kernels": {}}
    for name, mangled in KERNELS.items():
        insts = [i for _, _, x in ct_check.parse_function(asm, mangled) for i in x]
        b = [v for k, v in blocks.items() if mangled in k][0]
        out["kernels"][name] = dict(counts(insts), vgprs=int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)),
                                    private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    step = out["ladder_step"] = counts(longest_loop(asm, KERNELS["k_x25519"]))
    row = out["comb_row"] = counts(longest_loop(asm, KERNELS["k_x25519_base"]))
    out["ladder_step_mads_expected"] = 5 * MUL_MADS + 4 * SQR_MADS + SMALL_MADS + 2 * (10 + 4)
    inversion = out["inversion_valu"] = round((INVERT_SQR * SQR_MADS + INVERT_MUL * MUL_MADS) * step["valu"] / step["mads"])
    out["x25519_valu_per_lane"] = 255 * step["valu"] + (out["kernels"]["k_x25519"]["valu"] - step["valu"]) + inversion
    out["x25519_base_valu_per_lane"] = 64 * row["valu"] + (out["kernels"]["k_x25519_base"]["valu"] - row["valu"]) + inversion
    return out


if __name__ == "__main__":
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r14/x25519_listing.json is stale: python tools/x25519_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
