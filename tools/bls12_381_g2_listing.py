#!/usr/bin/env python3
"""bls12_381_listing.py's twin for the G2 unit: reads the shipped gfx950 listing of k_bls12_381_g2.hip
(build/csrc/k_bls12_381_g2-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes profiles/r22/bls12_381_g2_listing.json: per kernel the VALU and
multiply-add (v_mad_u64_u32) counts of its OWN text (loops counted once; the three point operations are out of line in this unit and are listed as functions of
their own, so a kernel's text does not hold them), its text size in bytes, the VGPR allocation (VGPRs and AGPRs are one 512-entry file per lane on gfx950; a
kernel's allocation covers the functions it calls) with the waves per SIMD it allows, scratch bytes and spills.

    python tools/bls12_381_g2_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                     # noqa: E402
from ed25519_listing import counts  # noqa: E402
from bls12_381_listing import waves_per_simd, dump, MUL_MADS  # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_bls12_381_g2-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r22", "bls12_381_g2_listing.json")
KERNELS = ("k_g2_decompress", "k_g2_compress", "k_g2_check", "k_g2_mul", "k_bls381_g2_raw", "k_g2_digits", "k_g2_slices", "k_g2_combine", "k_g2_chunks", "k_g2_tree",
           "k_g2_tree_affineILb0", "k_g2_tree_affineILb1", "k_g2_products", "k_g2_final")
FUNCTIONS = ("g2_dbl", "g2_add", "g2_madd")
FP2_MUL_MADS, FP2_SQR_MADS = 3 * MUL_MADS, 2 * MUL_MADS       # fp2.cuh: Karatsuba on three Fp products; the complex squaring on two


def info_after(asm, label):
    """The compiler's "; Kernel info:" / "; Function info:" block that follows the function `label`."""
    at = asm.index("\n" + label + ":")
    block = asm[asm.index(" info:\n", at):]
    block = block[:block.index("\n\t.")]
    return {k: int(v) for k, v in re.findall(r";\s+(\w+)[:=]?\s*=?\s*(\d+)\s*$", block, re.M)}


def report():
    asm = open(LISTING).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_bls12_381_g2.hip (tools/bls12_381_g2_listing.py).  g2_dbl, g2_add and g2_madd are OUT OF LINE: one copy of "
                      "each in the unit (`functions`), called by every kernel; a kernel's valu / mads are its own text without them, its registers and scratch "
                      "cover its callees.  Loops are counted once.  registers = the allocation out of the 512 per lane, with the waves per SIMD that allows.  By "
                      "the source an Fp2 product is 3 Fp products = 864 v_mad_u64_u32 and an Fp2 squaring 2 = 576; a mixed addition is 8 products and 3 squarings "
                      "= 8640, a doubling 2 + 5 = 4608, a general addition 12 + 4 = 12672.  predicted_mads_per_term_bucket_sum: one mixed addition per term and "
                      "window at bits = 255, c = 16 (16 windows): an instruction-count PREDICTION, not a measurement.",
           "kernels": {}, "functions": {}}
    for name in KERNELS:
        mangled = [k for k in blocks if re.search(r"\d" + re.escape(name) + "E", k)]    # the Itanium name: <length><name>E...
        assert len(mangled) == 1, (name, mangled)
        b = blocks[mangled[0]]
        insts = [i for _, _, x in ct_check.parse_function(asm, mangled[0]) for i in x]
        regs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        out["kernels"][name] = dict(counts(insts), text_bytes=info_after(asm, mangled[0])["codeLenInByte"], registers=regs, agprs=int(b.split()[0]),
                                    waves_per_simd=waves_per_simd(regs),
                                    private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    for name in FUNCTIONS:
        labels = re.findall(r"^(_ZN10ecsimd_hipL\d+" + name + r"E\w+):", asm, re.M)
        assert len(labels) == 1, (name, labels)
        insts = [i for _, _, x in ct_check.parse_function(asm, labels[0]) for i in x]
        info = info_after(asm, labels[0])
        out["functions"][name] = dict(counts(insts), text_bytes=info["codeLenInByte"], vgprs=info["NumVgprs"], agprs=info.get("NumAgprs", 0), scratch_bytes=info["ScratchSize"])
    out["mads"] = dict(fp2_product=FP2_MUL_MADS, fp2_squaring=FP2_SQR_MADS, mixed_addition=8 * FP2_MUL_MADS + 3 * FP2_SQR_MADS, doubling=2 * FP2_MUL_MADS + 5 * FP2_SQR_MADS,
                       addition=12 * FP2_MUL_MADS + 4 * FP2_SQR_MADS)
    out["predicted_mads_per_term_bucket_sum"] = 16 * out["mads"]["mixed_addition"]
    out["predicted_mads_per_term_lanes"] = 256 * out["mads"]["doubling"] + 128 * out["mads"]["mixed_addition"]
    return out


if __name__ == "__main__":
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r22/bls12_381_g2_listing.json is stale: python tools/bls12_381_g2_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(dump(r))
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
