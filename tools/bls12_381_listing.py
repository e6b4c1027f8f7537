#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of a BLS12-381 unit (build/csrc/k_bls12_381[_g2]-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r23/bls12_381_listing.json (--unit g1) or profiles/r23/bls12_381_g2_listing.json (--unit g2): per kernel the VALU and multiply-add (v_mad_u64_u32)
counts of its text (loops counted once), the VGPR allocation (VGPRs and AGPRs are one 512-entry file per lane on gfx950) with the waves per SIMD it allows,
scratch bytes and spills.  For G1 the aim was the bucket-sum kernels around ONE mixed addition (slices, tree_affine) at or below 256 registers with no scratch;
the file says what the compiler gave.  In the G2 unit the three point operations are out of line and are listed as functions of their own, so a kernel's text
does not hold them (its allocation covers the functions it calls), and every kernel's text size in bytes is recorded too.

Both units are k_bls12_381.inc's text: the kernels are k_g1_<stage> and k_g2_<stage>, and the units' own raw kernels k_bls381_raw and k_bls381_g2_raw.
profiles/r21/bls12_381_listing.json and profiles/r22/bls12_381_g2_listing.json are the listings of the two units as they were first written, each with its own
copy of the text; DESIGN.md 4n says what moved when the copies became one.

    python tools/bls12_381_listing.py [--unit g1|g2] [--check]      (no --unit: both; --check: compare with the committed files instead of writing them)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                     # noqa: E402
from ed25519_listing import counts  # noqa: E402

STAGES = ("decompress", "compress", "check", "mul", "raw", "digits", "slices", "combine", "chunks", "tree", "tree_affineILb0", "tree_affineILb1", "products", "final")
MUL_MADS, SQR_MADS = 288, 222       # fe381.cuh: 144 (78) for the double-width product, 144 for the Montgomery reduction
FP2_MUL_MADS, FP2_SQR_MADS = 3 * MUL_MADS, 2 * MUL_MADS       # fp2.cuh: Karatsuba on three Fp products; the complex squaring on two
UNITS = {
    "g1": dict(listing="k_bls12_381", out=os.path.join("profiles", "r23", "bls12_381_listing.json"), raw="k_bls381_raw", functions=(), product=MUL_MADS, squaring=SQR_MADS,
               comment="The shipped gfx950 listing of k_bls12_381.hip (tools/bls12_381_listing.py --unit g1).  Per kernel: VALU instructions and v_mad_u64_u32 in its TEXT "
                       "(loops counted once), registers = the allocation out of the 512 per lane, the waves per SIMD that allows, scratch bytes.  By the source a "
                       "field product is 288 v_mad_u64_u32 (144 for the columns, 144 for the Montgomery reduction) and a squaring 222; a mixed addition is 8 products "
                       "and 3 squarings = 2970, a doubling 2 + 5 = 1686, a general addition 12 + 4 = 4344.  predicted_mads_per_term_bucket_sum: one mixed "
                       "addition per term and window at bits = 255, c = 16 (16 windows): an instruction-count PREDICTION, not a measurement."),
    "g2": dict(listing="k_bls12_381_g2", out=os.path.join("profiles", "r23", "bls12_381_g2_listing.json"), raw="k_bls381_g2_raw", functions=("g2_dbl", "g2_add", "g2_madd"),
               product=FP2_MUL_MADS, squaring=FP2_SQR_MADS,
               comment="The shipped gfx950 listing of k_bls12_381_g2.hip (tools/bls12_381_listing.py --unit g2).  g2_dbl, g2_add and g2_madd are OUT OF LINE: one copy of "
                       "each in the unit (`functions`), called by every kernel; a kernel's valu / mads are its own text without them, its registers and scratch "
                       "cover its callees.  Loops are counted once.  registers = the allocation out of the 512 per lane, with the waves per SIMD that allows.  By "
                       "the source an Fp2 product is 3 Fp products = 864 v_mad_u64_u32 and an Fp2 squaring 2 = 576; a mixed addition is 8 products and 3 squarings "
                       "= 8640, a doubling 2 + 5 = 4608, a general addition 12 + 4 = 12672.  predicted_mads_per_term_bucket_sum: one mixed addition per term and "
                       "window at bits = 255, c = 16 (16 windows): an instruction-count PREDICTION, not a measurement."),
}


def waves_per_simd(registers):
    """gfx950: 512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves."""
    return max(1, min(8, 512 // ((registers + 7) // 8 * 8)))


def info_after(asm, label):
    """The compiler's "; Kernel info:" / "; Function info:" block that follows the function `label`."""
    at = asm.index("\n" + label + ":")
    block = asm[asm.index(" info:\n", at):]
    block = block[:block.index("\n\t.")]
    return {k: int(v) for k, v in re.findall(r";\s+(\w+)[:=]?\s*=?\s*(\d+)\s*$", block, re.M)}


def kernel_of(unit, stage):
    """A stage's kernel in `unit`, which is also its key in the file: k_g1_<stage>, k_g2_<stage>, and the raw kernels' own names."""
    return UNITS[unit]["raw"] if stage == "raw" else "k_%s_%s" % (unit, stage)


def report(unit, listing=None):
    U = UNITS[unit]
    asm = open(listing or os.path.join(ROOT, "build", "csrc", U["listing"] + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": U["comment"], "kernels": {}}
    for stage in STAGES:
        key = kernel_of(unit, stage)
        mangled = [k for k in blocks if re.search(r"\d" + re.escape(key) + "E", k)]    # the Itanium name: <length><name>E...
        assert len(mangled) == 1, (stage, mangled)
        b = blocks[mangled[0]]
        insts = [i for _, _, x in ct_check.parse_function(asm, mangled[0]) for i in x]
        regs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        text = dict(text_bytes=info_after(asm, mangled[0])["codeLenInByte"]) if U["functions"] else {}
        out["kernels"][key] = dict(counts(insts), **text, registers=regs, agprs=int(b.split()[0]), waves_per_simd=waves_per_simd(regs),
                                   private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                   vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                   lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    if U["functions"]:
        out["functions"] = {}
    for name in U["functions"]:
        labels = re.findall(r"^(_ZN10ecsimd_hipL\d+" + name + r"E\w+):", asm, re.M)
        assert len(labels) == 1, (name, labels)
        insts = [i for _, _, x in ct_check.parse_function(asm, labels[0]) for i in x]
        info = info_after(asm, labels[0])
        out["functions"][name] = dict(counts(insts), text_bytes=info["codeLenInByte"], vgprs=info["NumVgprs"], agprs=info.get("NumAgprs", 0), scratch_bytes=info["ScratchSize"])
    P, S = U["product"], U["squaring"]
    pre = "fp2_" if unit == "g2" else ""
    out["mads"] = {pre + "product": P, pre + "squaring": S, "mixed_addition": 8 * P + 3 * S, "doubling": 2 * P + 5 * S, "addition": 12 * P + 4 * S}
    out["predicted_mads_per_term_bucket_sum"] = 16 * out["mads"]["mixed_addition"]
    out["predicted_mads_per_term_lanes"] = 256 * out["mads"]["doubling"] + 128 * out["mads"]["mixed_addition"]
    return out


def dump(r):
    """One kernel per line."""
    line = lambda v: json.dumps(v, separators=(", ", ": "))
    body = ",\n".join(' %s: {\n%s\n }' % (json.dumps(k), ",\n".join('  %s: %s' % (json.dumps(n), line(c)) for n, c in v.items())) if k == "kernels" else ' %s: %s' % (json.dumps(k), line(v))
                      for k, v in r.items())
    return "{\n" + body + "\n}\n"


if __name__ == "__main__":
    units = [sys.argv[sys.argv.index("--unit") + 1]] if "--unit" in sys.argv else ["g1", "g2"]
    for unit in units:
        r, out = report(unit), os.path.join(ROOT, UNITS[unit]["out"])
        if "--check" in sys.argv:
            assert json.load(open(out)) == r, "%s is stale: python tools/bls12_381_listing.py --unit %s" % (UNITS[unit]["out"], unit)
        else:
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "w") as f:
                f.write(dump(r))
        print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
