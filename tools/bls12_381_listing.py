#!/usr/bin/env python3
"""Reads the shipped gfx950 listing of k_bls12_381.hip (build/csrc/k_bls12_381-hip-amdgcn-amd-amdhsa-gfx950.s, left there by the Makefile) and writes
profiles/r21/bls12_381_listing.json: per kernel the VALU and multiply-add (v_mad_u64_u32) counts of its text (loops counted once), the VGPR allocation (VGPRs
and AGPRs are one 512-entry file per lane on gfx950) with the waves per SIMD it allows, scratch bytes and spills.  The aim was the bucket-sum kernels around
ONE mixed addition (slices, tree_affine) at or below 256 registers with no scratch; the file says what the compiler gave.

    python tools/bls12_381_listing.py [--check]      (--check: compare with the committed file instead of writing it)
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_check                     # noqa: E402
from ed25519_listing import counts  # noqa: E402

LISTING = os.path.join(ROOT, "build", "csrc", "k_bls12_381-hip-amdgcn-amd-amdhsa-gfx950.s")
OUT = os.path.join(ROOT, "profiles", "r21", "bls12_381_listing.json")
KERNELS = ("k_g1_decompress", "k_g1_compress", "k_g1_check", "k_g1_mul", "k_bls381_raw", "k_g1_digits", "k_g1_slices", "k_g1_combine", "k_g1_chunks", "k_g1_tree",
           "k_g1_tree_affineILb0", "k_g1_tree_affineILb1", "k_g1_products", "k_g1_final")
MUL_MADS, SQR_MADS = 288, 222       # fe381.cuh: 144 (78) for the double-width product, 144 for the Montgomery reduction


def waves_per_simd(registers):
    """gfx950: 512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves."""
    return max(1, min(8, 512 // ((registers + 7) // 8 * 8)))


def report():
    asm = open(LISTING).read()
    meta = asm[asm.index(".amdgpu_metadata"):]
    blocks = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in re.split(r"\n  - \.agpr_count:", meta)[1:]}
    out = {"comment": "The shipped gfx950 listing of k_bls12_381.hip (tools/bls12_381_listing.py).  Per kernel: VALU instructions and v_mad_u64_u32 in its TEXT "
                      "(loops counted once), registers = the allocation out of the 512 per lane, the waves per SIMD that allows, scratch bytes.  By the source a "
                      "field product is 288 v_mad_u64_u32 (144 for the columns, 144 for the Montgomery reduction) and a squaring 222; a mixed addition is 8 products "
                      "and 3 squarings = 2970, a doubling 2 + 5 = 1686, a general addition 12 + 4 = 4344.  predicted_mads_per_term_bucket_sum: one mixed "
                      "addition per term and window at bits = 255, c = 16 (16 windows): an instruction-count PREDICTION, not a measurement.",
           "kernels": {}}
    for name in KERNELS:
        mangled = [k for k in blocks if re.search(r"\d" + re.escape(name) + "E", k)]    # the Itanium name: <length><name>E...
        assert len(mangled) == 1, (name, mangled)
        b = blocks[mangled[0]]
        insts = [i for _, _, x in ct_check.parse_function(asm, mangled[0]) for i in x]
        regs = int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1))
        out["kernels"][name] = dict(counts(insts), registers=regs, agprs=int(b.split()[0]), waves_per_simd=waves_per_simd(regs),
                                    private_segment_fixed_size=int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)),
                                    vgpr_spill_count=int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)),
                                    lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)))
    out["mads"] = dict(product=MUL_MADS, squaring=SQR_MADS, mixed_addition=8 * MUL_MADS + 3 * SQR_MADS, doubling=2 * MUL_MADS + 5 * SQR_MADS, addition=12 * MUL_MADS + 4 * SQR_MADS)
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
    r = report()
    if "--check" in sys.argv:
        assert json.load(open(OUT)) == r, "profiles/r21/bls12_381_listing.json is stale: python tools/bls12_381_listing.py"
    else:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(dump(r))
    print(json.dumps({k: v for k, v in r.items() if k != "comment"}, indent=1))
