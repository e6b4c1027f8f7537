#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of k_sm2.hip (build/csrc/k_sm2-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r20/sm2_listing.json: per kernel the VALU count of its text, the VGPR allocation with the waves per SIMD it allows, scratch and LDS; and the VALU
instructions of ONE SM3 compression -- the text of the shortest loop of k_sm3 that holds a whole compression (the padding loop: a block of registers, the
bit length, the 64 rounds).

    python tools/sm2_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                                   # noqa: E402
from ed25519_listing import counts                # noqa: E402
from p384_listing import dump, waves_per_simd     # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_sm2-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r20", "sm2_listing.json")
KERNELS = ("k_sm3", "k_sm2_za", "k_sm2_digest", "k_sm2_verify_scalars", "k_sm2_accept", "k_sm2_sign_scalars", "k_sm2_key_range")
ROUNDS = 64


def loops(asm, kernel):
    """The instruction lists between the target label and the backward branch of every loop of `kernel`."""
    start, flat = {}, []
    for label, _, insts in ct_check.parse_function(asm, kernel):
        start[label] = len(flat)
        flat += insts
    out = []
    for i, t in enumerate(flat):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", t) or re.match(r"s_branch\s+(\S+)", t)
        if m and m.group(1) in start and start[m.group(1)] <= i:
            out.append(flat[start[m.group(1)]:i + 1])
    return out


def report(asm=None):
    asm = open(LISTING).read() if asm is None else asm
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_sm2.hip (tools/sm2_listing.py).  Per kernel: VALU instructions in its TEXT (loops counted once; k_sm3 and "
                      "k_sm2_digest hold the walker twice, for word and for byte loads), the VGPR allocation, the waves per SIMD it allows, scratch and LDS bytes.  "
                      "valu_per_compression: the text of the shortest loop of k_sm3 with a whole compression in it -- a register block, the bit length, the 64 "
                      "rounds; rotations_per_compression its v_alignbit_b32, bit_selects its v_bfi_b32 / v_bitop3_b32.",
           "kernels": {}}
    for name in KERNELS:
        insts = [i for _, _, x in ct_check.parse_function(asm, "_GLOBAL__N_1%d%sE" % (len(name), name)) for i in x]
        b = [v for k, v in blocks.items() if "_GLOBAL__N_1%d%sE" % (len(name), name) in k][0]
        regs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        out["kernels"][name] = dict(valu=counts(insts)["valu"], vmem=counts(insts)["vmem"], vgprs=regs, sgprs=int(re.search(r"\.sgpr_count:\s+(\d+)", b).group(1)),
                                    waves_per_simd=waves_per_simd(regs), scratch_bytes=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    whole = [body for body in loops(asm, "_GLOBAL__N_15k_sm3E") if sum(1 for i in body if i.startswith("v_alignbit_b32")) >= 4 * ROUNDS]
    best = min(whole, key=lambda body: counts(body)["valu"])
    out["valu_per_compression"] = counts(best)["valu"]
    out["rotations_per_compression"] = sum(1 for i in best if i.startswith("v_alignbit_b32"))
    out["bit_selects_per_compression"] = sum(1 for i in best if i.startswith(("v_bfi_b32", "v_bitop3_b32")))
    out["adds_per_compression"] = sum(1 for i in best if i.startswith(("v_add_u32", "v_add3_u32", "v_add_co")))
    return out


if __name__ == "__main__":
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r20/sm2_listing.json is stale: python tools/sm2_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(dump(r))
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
