#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of k_ed25519.hip (build/csrc/k_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r13/ed25519_listing.json: per kernel the VALU and multiply (v_mad_u64_u32) counts and the registers; for the two scalar-multiplication loops the
counts of the loop body (the text between the label and the closing backward branch of the kernel's longest loop); and the a-priori figures they imply --
field multiplications and VALU instructions per verification -- to hold the measured rate of tools/time_ed25519.py against.

    python tools/ed25519_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check   # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_ed25519-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r13", "ed25519_listing.json")
KERNELS = {"k_ed_secret_front<false>": "k_ed_secret_frontILb0E", "k_ed_secret_front<true>": "k_ed_secret_frontILb1E", "k_ed_base_ct": "k_ed_base_ct",
           "k_ed_sign_finish": "k_ed_sign_finish", "k_ed_verify_front": "k_ed_verify_front", "k_ed_verify_loop": "k_ed_verify_loop", "k_ed_raw": "k_ed_raw"}
MUL_MADS, SQR_MADS = 72, 44        # fe25519_mul: 64 column products + 8 of the fold by 38; fe25519_sqr: 28 + 8 + 8


def counts(insts):
    c = collections.Counter(i.split()[0] for i in insts)
    return dict(valu=sum(v for k, v in c.items() if k.startswith("v_")), mads=c["v_mad_u64_u32"], moves=c["v_mov_b32_e32"] + c["v_mov_b64_e32"],
                vmem=sum(v for k, v in c.items() if k.startswith(("global_", "buffer_", "flat_", "scratch_"))))


def longest_loop(asm, kernel):
    """The instructions between the target label and the backward branch of the longest loop of `kernel`."""
    blocks = ct_check.parse_function(asm, kernel)
    start, flat = {}, []
    for label, _, insts in blocks:
        start[label] = len(flat)
        flat += insts
    best = (0, 0)
    for i, t in enumerate(flat):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", t) or re.match(r"s_branch\s+(\S+)", t)
        if m and m.group(1) in start and start[m.group(1)] <= i and i + 1 - start[m.group(1)] > best[1] - best[0]:
            best = (start[m.group(1)], i + 1)
    return flat[best[0]:best[1]]


def report():
    asm = open(LISTING).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_ed25519.hip (tools/ed25519_listing.py).  Per kernel: VALU instructions and v_mad_u64_u32 in its text, "
                      "VGPRs, scratch and LDS bytes.  verify_loop_body / comb_loop_body: the body of the kernel's longest loop -- one position of the "
                      "verification loop (four doublings, both additions in its text) and one row of the comb (one selection over eight entries, one mixed "
                      "addition).  A field multiplication is 72 v_mad_u64_u32 (64 column products, 8 of the fold by 38), a squaring 44.  "
                      "verify_field_multiplications: 64 positions x (16 squarings + 13 products of the doublings + 15/16 x 7 + 15/16 x 8 of the two additions, a "
                      "digit being 0 once in 16) + the 7 additions of the table + the encoding's 254 squarings and 13 products + the decoding's 253 and 20, "
                      "squarings counted as 44/72 of a product.  verify_valu_per_lane: 64 x the loop body's VALU with both additions taken + the rest of "
                      "both kernels' text once (every loop of the inversion chains is a few squarings: its text is an upper bound of nothing and a lower bound "
                      "of little; the figure is a-priori, not a measurement).  No rate has been measured yet: profiles/r13/ed25519.txt is tools/time_ed25519.py's to write.",
           "kernels": {}}
    for name, mangled in KERNELS.items():
        insts = [i for _, _, x in ct_check.parse_function(asm, mangled) for i in x]
        b = [v for k, v in blocks.items() if mangled in k][0]
        out["kernels"][name] = dict(counts(insts), vgprs=int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)),
                                    private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    out["verify_loop_body"] = counts(longest_loop(asm, "k_ed_verify_loop"))
    out["comb_loop_body"] = counts(longest_loop(asm, "k_ed_base_ct"))
    sq = SQR_MADS / MUL_MADS
    loop = 64 * (16 * sq + 13 + 15 / 16 * 7 + 15 / 16 * 8)
    rest = 7 * 9 + (254 * sq + 13) + (253 * sq + 20)
    out["verify_field_multiplications"] = round(loop + rest)
    out["verify_loop_mads_expected"] = 16 * SQR_MADS + (13 + 7 + 8) * MUL_MADS
    out["verify_valu_per_lane"] = 64 * out["verify_loop_body"]["valu"] + (out["kernels"]["k_ed_verify_loop"]["valu"] - out["verify_loop_body"]["valu"]) + out["kernels"]["k_ed_verify_front"]["valu"]
    out["sign_field_multiplications"] = round(2 * (64 * 7 + 3 * (4 * sq + 3) + (4 * sq + 4) + 254 * sq + 13))
    return out


if __name__ == "__main__":
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r13/ed25519_listing.json is stale: python tools/ed25519_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
